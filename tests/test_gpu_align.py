"""Alignment on the MI355X: find_align_fit / find_icp_run through find_amd.align against the float64 numpy restatement of the rules
(tests/align_ref.py) on the same fp32 inputs, and their place in init_registration, eval_metrics and evaluate.eval_3d.

Margins: none is a constant of the code under test.  Every float comparison follows tests/test_gpu_measure.py's _held: the same reference is
also evaluated in float32 on the CPU; with e32 its worst error against float64 over the case's tensor, the HIP result must lie within
max(4 e32, 2 ulp of the largest value) of the float64 one.  Where nearest neighbours are compared as integers, the generator redraws queries
until, in float64, every query's best and second-best d2 differ by at least 1e-5 extent^2 -- about 25 times the ~4e-7 extent^2 by which an
fp32 d2 can be off -- so the indices must be equal.  Each case prints its figures (DESIGN 7.10 records the worst).

Shapes: clouds uniform in a 0.25 x 0.10 x 0.08 box (a foot's proportions); a workgroup takes 256 pairs, a wave 64.  P = 4, 63, 64, 65, 255, 256,
257, 1000 (below a wave, around one, around a workgroup, several workgroups); N = 1, and N = 3 ragged with a last cloud of length 2, which
must come back as the identity (inside ICP: the transform it started from) with status bit 2 and no NaN; one 8192 x 8192 step, the size
from which the Chamfer search leaves all pairs (find_nn_fwd itself has the one path: 64 workgroups of queries there, 32 of moments).
Every case runs twice and must repeat bit for bit."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_ref as ref   # noqa: E402
import poison   # noqa: E402

SIZES = (4, 63, 64, 65, 255, 256, 257, 1000)
BOX = np.array([0.25, 0.10, 0.08])
EXTENT2 = float((BOX ** 2).sum())
ITERS = 30
WORST = {}   # name of a quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip = hip.detach().double().cpu() if torch.is_tensor(hip) else torch.as_tensor(np.asarray(hip, dtype=np.float64))
	ref64, ref32 = torch.as_tensor(np.asarray(ref64, dtype=np.float64)), torch.as_tensor(np.asarray(ref32, dtype=np.float64))
	assert hip.shape == ref64.shape == ref32.shape, (name, hip.shape, ref64.shape, ref32.shape)
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs
def _lens(P, floor=4):
	"""N = 1: the whole cloud; N = 3: ragged, the last cloud of length 2."""
	return {1: [P], 3: [P, max(floor, 2 * P // 3), 2]}


def _box(rng, P):
	return (rng.random((P, 3)) * BOX).astype(np.float32)


def _pad(clouds, fill=np.nan):
	"""A list of (p_n, 3) fp32 clouds -> (N, p_max, 3) with rows past a cloud's end holding `fill` (they are never read), and the lengths."""
	p_max = max(len(c) for c in clouds)
	out = np.full((len(clouds), p_max, 3), fill, dtype=np.float32)
	for n, c in enumerate(clouds):
		out[n, :len(c)] = c
	return torch.from_numpy(out), torch.tensor([len(c) for c in clouds], dtype=torch.int32)


def _truth(rng, degrees, t_mm, s=1.):
	return ref.rotation(rng.normal(size=3), math.radians(degrees)), np.asarray(t_mm, dtype=np.float64) * 1e-3, float(s)


def _tr(sol_or_tr, n):
	"""(R, t, s) of cloud n as float64 numpy."""
	R, T, s = sol_or_tr
	return R[n].double().cpu().numpy(), T[n].double().cpu().numpy(), float(s[n])


def _same(a, b, what):
	"""Two runs of one call: every tensor bit for bit."""
	for k, (u, v) in enumerate(zip(a, b)):
		if isinstance(u, tuple):
			_same(u, v, f'{what}[{k}]')
		else:
			assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u.view(torch.int32) if u.is_floating_point() else u, v.view(torch.int32) if v.is_floating_point() else v), (what, k)


def _icp(X, Y, x_len=None, y_len=None, **kw):
	"""iterative_closest_point twice: the two runs must agree bit for bit."""
	from find_amd.align import iterative_closest_point
	args = (X.cuda(), Y.cuda(), None if x_len is None else x_len.cuda(), None if y_len is None else y_len.cuda())
	a, b = iterative_closest_point(*args, **kw), iterative_closest_point(*args, **kw)
	torch.cuda.synchronize()
	_same(a, b, 'iterative_closest_point')
	assert a.rmse.dtype == torch.float32 and a.idx.dtype == a.iterations.dtype == a.status.dtype == a.used.dtype == torch.int32 and a.converged.dtype == torch.bool
	assert all(torch.isfinite(t).all() for t in (a.rmse, a.Xt, a.dist, *a.RTs)) and not any(t.requires_grad for t in (a.rmse, a.Xt, *a.RTs))
	return a


def _stack(outs, key):
	return np.stack([np.asarray(o[key], dtype=np.float64) for o in outs])


# ------------------------------------------------------------------ the fit alone
def _fit_case(P, N, mode, weighted, seed):
	"""Pairs of a known transform plus 1 mm of noise; Y mirrored for mode 'reflection'."""
	rng = np.random.default_rng(seed)
	xs, ys, ws = [], [], []
	for p in _lens(P)[N]:
		x = _box(rng, p)
		R0, t0, s0 = _truth(rng, 40 * rng.random() + 5, 30 * rng.normal(size=3), 0.8 + 0.4 * rng.random() if mode != 'rigid' else 1.)
		if mode == 'reflection':
			R0 = R0 * np.array([-1., 1., 1.])[:, None]
		xs.append(x)
		ys.append((ref.apply(x.astype(np.float64), R0, t0, s0) + 1e-3 * rng.normal(size=(p, 3))).astype(np.float32))
		w = (rng.random(p) + 0.25).astype(np.float32)
		if p >= 8:
			w[rng.permutation(p)[:p // 4]] = 0
		ws.append(w)
	X, lens = _pad(xs)
	Y, _ = _pad(ys)
	W = None
	if weighted:
		W = torch.full(X.shape[:2], float('nan'))
		for n, w in enumerate(ws):
			W[n, :len(w)] = torch.from_numpy(w)
	return xs, ys, (ws if weighted else [None] * len(xs)), X, Y, W, lens


@pytest.mark.parametrize('P', SIZES)
@pytest.mark.parametrize('N', (1, 3))
def test_fit_against_float64(P, N):
	from find_amd.align import corresponding_points_alignment
	for mode in ('rigid', 'similarity', 'reflection'):
		for weighted in (False, True):
			xs, ys, ws, X, Y, W, lens = _fit_case(P, N, mode, weighted, seed=100 * P + 10 * N + weighted)
			kw = dict(estimate_scale=mode != 'rigid', allow_reflection=mode == 'reflection')
			args = (X.cuda(), Y.cuda(), None if W is None else W.cuda())
			got = corresponding_points_alignment(*args, lengths=lens.cuda() if N > 1 else None, return_status=True, **kw)
			again = corresponding_points_alignment(*args, lengths=lens.cuda() if N > 1 else None, return_status=True, **kw)
			torch.cuda.synchronize()
			_same(got, again, 'corresponding_points_alignment')
			tr, status = got
			assert all(torch.isfinite(t).all() for t in tr)
			r64 = [ref.umeyama(x, y, w, dtype=np.float64, **kw) for x, y, w in zip(xs, ys, ws)]
			r32 = [ref.umeyama(x, y, w, dtype=np.float32, **kw) for x, y, w in zip(xs, ys, ws)]
			tag = f'fit P={P} N={N} {mode}{" weighted" if weighted else ""}'
			assert status.cpu().tolist() == [r[3] for r in r64] == [0] * (N - 1) + [2 if N == 3 else 0], tag
			for k, (what, t) in enumerate(zip('Rts', tr)):
				_held(f'{tag} {what}', t, np.stack([r[k] for r in r64]), np.stack([r[k] for r in r32]), kind='fit ' + what)
			R = tr.R.double().cpu()
			R32 = torch.as_tensor(np.stack([r[0] for r in r32]).astype(np.float64))
			eye = torch.eye(3, dtype=torch.float64).expand(N, 3, 3)
			_held(f'{tag} R^T R', R.transpose(1, 2) @ R, eye, R32.transpose(1, 2) @ R32, kind='fit RtR')
			det = torch.linalg.det(R)
			want = torch.tensor([-1. if mode == 'reflection' and s == 0 else 1. for s in status.cpu().tolist()], dtype=torch.float64)
			_held(f'{tag} det', det, want, torch.linalg.det(R32), kind='fit det')
			if N == 3:   # the cloud of two pairs: identity
				assert torch.equal(tr.R[2].cpu(), torch.eye(3)) and not tr.T[2].any() and tr.s[2].item() == 1.


def test_fit_refuses_degenerate_pairs_and_ignores_weightless_rows():
	from find_amd.align import corresponding_points_alignment
	rng = np.random.default_rng(8)
	x = torch.from_numpy(_box(rng, 300))
	line = torch.outer(torch.arange(300.), torch.tensor([1., 2., 3.])) * 2. ** -10   # (exact in fp32: exactly collinear)
	X = torch.stack([x, line, torch.ones(300, 3), x, x])
	Y = torch.stack([x.flip(0), x, x, x * float('nan'), x + 1.])
	W = torch.ones(5, 300)
	W[3] = 0                  # no pair of positive weight: its NaN rows are never read
	W[4, 2:] = -1.            # two pairs of positive weight
	tr, status = corresponding_points_alignment(X.cuda(), Y.cuda(), W.cuda(), estimate_scale=True, return_status=True)
	assert status.cpu().tolist() == [0, 2, 2, 2, 2]
	for n in range(1, 5):
		assert torch.equal(tr.R[n].cpu(), torch.eye(3)) and not tr.T[n].any() and tr.s[n].item() == 1., n
	assert all(torch.isfinite(t).all() for t in tr)
	# a row of weight 0 may hold anything, row 0 (the pivot) included
	Xn, Yn, Wn = X[:1].clone(), Y[:1].clone(), torch.ones(1, 300)
	Wn[0, [0, 17]] = 0
	clean = corresponding_points_alignment(Xn[:, torch.arange(300) != 17][:, 1:].contiguous().cuda(), Yn[:, torch.arange(300) != 17][:, 1:].contiguous().cuda())
	Xn[0, [0, 17]] = float('nan')
	Yn[0, 17] = float('inf')
	dirty = corresponding_points_alignment(Xn.cuda(), Yn.cuda(), Wn.cuda())
	assert all(torch.isfinite(t).all() for t in dirty)
	for a, b in zip(clean, dirty):   # (other pivots, another split into workgroups: equal to fp32's resolution, not to the bit)
		assert torch.allclose(a, b, rtol=0, atol=2 * _ulp(1.))


# ------------------------------------------------------------------ one step of the loop
def _step_case(lens1, lens2, seed):
	rng = np.random.default_rng(seed)
	xs, ys, inits, d2s, idxs = [], [], [], [], []
	for p1, p2 in zip(lens1, lens2):
		y = _box(rng, p2)
		R0, t0, s0 = _truth(rng, 25, 20 * rng.normal(size=3), 1.1)
		# the queries: y's own box seen through the inverse of the init transform, so that the match is not trivial
		init = (R0.astype(np.float32), t0.astype(np.float32), np.float32(s0))
		i64 = tuple(np.asarray(v, dtype=np.float64) for v in init)
		x = (((_box(rng, p1).astype(np.float64) - i64[1]) / i64[2]) @ i64[0].T).astype(np.float32)

		def redraw(r, k, i64=i64):
			return (((_box(r, k).astype(np.float64) - i64[1]) / i64[2]) @ i64[0].T).astype(np.float32)
		x, d2, idx = _separated_with(rng, x, y, i64, 1e-5 * EXTENT2, redraw)
		xs.append(x); ys.append(y); inits.append(init); d2s.append(d2); idxs.append(idx)
	return xs, ys, inits, d2s, idxs


def _separated_with(rng, x, y, init, floor, redraw):
	"""Redraw the queries of x (p1, 3) fp32 whose nearest and second-nearest y under `init`, in float64, are closer than `floor` in d2.
	Returns x and, in float64, its d2 and nearest indices."""
	R, t, s = init
	y64 = y.astype(np.float64)
	bad = np.arange(len(x))
	for _ in range(500):
		a, _, b = ref.nearest(ref.apply(x[bad].astype(np.float64), R, t, s), y64, second=True)
		bad = bad[b - a < floor]
		if not len(bad):
			break
		x[bad] = redraw(rng, len(bad))
	a, j, b = ref.nearest(ref.apply(x.astype(np.float64), R, t, s), y64, second=True)
	assert (b - a >= floor).all(), (b - a).min()
	return x, a, j


def _one_step(tag, lens1, lens2, seed):
	from find_amd.align import SimilarityTransform
	xs, ys, inits, d2s, idxs = _step_case(lens1, lens2, seed)
	X, xl = _pad(xs)
	Y, yl = _pad(ys)
	N = len(xs)
	init = SimilarityTransform(torch.from_numpy(np.stack([i[0] for i in inits])).cuda(), torch.from_numpy(np.stack([i[1] for i in inits])).cuda(),
							   torch.from_numpy(np.stack([i[2] for i in inits])).cuda())
	ragged = dict(x_len=xl, y_len=yl) if N > 1 else {}
	# no update: the match under the init transform itself
	m = _icp(X, Y, init_transform=init, max_iterations=0, **ragged)
	assert m.status.cpu().tolist() == [1] * N and m.iterations.cpu().tolist() == [0] * N
	_same(tuple(m.RTs), tuple(init), 'the transform of max_iterations = 0')
	for n in range(N):
		p1 = len(xs[n])
		assert np.array_equal(m.idx[n, :p1].cpu().numpy(), idxs[n]), (tag, n)
		assert (m.idx[n, p1:] == -1).all() and (m.dist[n, p1:] == 0).all() and (m.Xt[n, p1:] == 0).all()
		d32, _ = ref.nearest(ref.apply(xs[n], *inits[n]).astype(np.float32), ys[n])
		_held(f'{tag} cloud {n} d2', m.dist[n, :p1], d2s[n], d32, kind='step d2')
		assert m.used[n].item() == p1 and math.isinf(m.tau[n].item())
	# one update from those matches
	got = _icp(X, Y, init_transform=init, max_iterations=1, estimate_scale=True, **ragged)
	r64 = [ref.icp(x, y, init=i, max_iterations=1, estimate_scale=True, dtype=np.float64) for x, y, i in zip(xs, ys, inits)]
	r32 = [ref.icp(x, y, init=i, max_iterations=1, estimate_scale=True, dtype=np.float32) for x, y, i in zip(xs, ys, inits)]
	assert got.iterations.cpu().tolist() == [r['iterations'] for r in r64], tag
	assert [s & 2 for s in got.status.cpu().tolist()] == [r['status'] & 2 for r in r64], tag
	for what, t, key in (('R', got.RTs.R, 'R'), ('t', got.RTs.T, 't'), ('s', got.RTs.s, 's')):
		_held(f'{tag} {what}', t, _stack(r64, key), _stack(r32, key), kind='step ' + what)
	return got, r64


@pytest.mark.parametrize('P', SIZES)
@pytest.mark.parametrize('N', (1, 3))
def test_one_step_against_float64(P, N):
	lens1 = _lens(P)[N]
	lens2 = [P + 3, max(4, P // 2), 5][:N]
	got, r64 = _one_step(f'step P={P} N={N}', lens1, lens2, seed=7000 + 10 * P + N)
	if N == 3:   # two queries: nothing to solve, the init transform stays
		assert got.status[2].item() & 2 and got.iterations[2].item() == 0 and r64[2]['status'] & 2


def test_one_step_at_8192():
	"""8192 queries and targets in one cloud, the size at which the Chamfer search switches to its grid: the loop's match is find_nn_fwd,
	which stays with all pairs (64 workgroups of queries); 32 workgroups of moments.  One step: the float64 reference is chunked on the CPU."""
	_one_step('step 8192', [8192], [8192], seed=8192)


# ------------------------------------------------------------------ the select
@pytest.mark.parametrize('P', SIZES)
def test_select_is_the_kth_smallest(P):
	rng = np.random.default_rng(300 + P)
	clouds = [_box(rng, P), np.repeat(_box(rng, (P + 3) // 4), 4, axis=0)[:P], _box(rng, max(4, P // 2))]   # the second: every point four times (ties)
	X, xl = _pad(clouds)
	Y, yl = _pad([_box(rng, P + 1), np.repeat(_box(rng, P // 2 + 1), 2, axis=0), _box(rng, 7)])
	for name, trim_of in (('k = 1', lambda m: (m - 0.5) / m), ('k = m', lambda m: 0.5 / m), ('0.2', lambda m: 0.2), ('0.5', lambda m: 0.5), ('0.93', lambda m: 0.93)):
		trim = trim_of(P)   # (k = 1 and k = m: of the first cloud)
		sol = _icp(X, Y, x_len=xl, y_len=yl, max_iterations=0, trim=trim)
		for n, m in enumerate(xl.tolist()):
			k = ref.keep_count(m, trim)
			d = sol.dist[n, :m]
			kth = torch.sort(d).values[k - 1]
			assert sol.tau[n].view(torch.int32).item() == kth.view(torch.int32).item(), (P, name, n, sol.tau[n].item(), kth.item())
			assert sol.used[n].item() == int((d <= sol.tau[n]).sum()) >= k, (P, name, n)
			if n == 0 and name in ('k = 1', 'k = m'):
				assert k == (1 if name == 'k = 1' else m)
		# with a distance limit: both conditions
		lim = float(sol.dist[0, :P].median().sqrt())
		if lim > 0:
			cut = _icp(X, Y, x_len=xl, y_len=yl, max_iterations=0, trim=trim, max_distance=lim)
			lim2 = torch.tensor(lim, dtype=torch.float32) ** 2
			for n, m in enumerate(xl.tolist()):
				d = cut.dist[n, :m].cpu()
				assert torch.equal(cut.tau[n], sol.tau[n]) and cut.used[n].item() == int(((d <= cut.tau[n].cpu()) & (d <= lim2)).sum()), (P, name, n)


# ------------------------------------------------------------------ the whole loop
def _copy_case(P, N, seed, degrees, t_mm, s, floor):
	rng = np.random.default_rng(seed)
	xs, ys, truths = [], [], []
	for p in _lens(P, floor)[N]:
		x = _box(rng, p)
		R0, t0, s0 = _truth(rng, degrees, t_mm, s)
		xs.append(x)
		ys.append(ref.apply(x.astype(np.float64), R0, t0, s0)[rng.permutation(p)].astype(np.float32))
		truths.append(dict(R=R0, t=t0, s=s0))
	return xs, ys, truths


def _whole_loop(tag, xs, ys, truths, skip=(), **kw):
	"""ICP on the clouds as one ragged batch against the float64 and float32 references and the truth; `skip`: clouds that are too small to
	say anything about (they only ride along)."""
	X, xl = _pad(xs)
	Y, yl = _pad(ys)
	N = len(xs)
	r64 = [ref.icp(x, y, max_iterations=ITERS, dtype=np.float64, **{('max_dist' if k == 'max_distance' else k): v for k, v in kw.items()}) for x, y in zip(xs, ys)]
	r32 = [ref.icp(x, y, max_iterations=ITERS, dtype=np.float32, **{('max_dist' if k == 'max_distance' else k): v for k, v in kw.items()}) for x, y in zip(xs, ys)]
	keep = [n for n in range(N) if n not in skip]
	for n in keep:   # the generator's claim: the float64 reference converged, to the truth
		assert r64[n]['status'] == 0 and r64[n]['iterations'] < ITERS and r64[n]['rmse'] < 1e-7, (tag, n, r64[n]['status'], r64[n]['iterations'], r64[n]['rmse'])
		print(f'{tag} cloud {n}: float64 reference: {r64[n]["iterations"]} iterations, rmse {r64[n]["rmse"]:.2e}, rotation error {ref.rotation_error(r64[n]["R"], truths[n]["R"]):.2e}')
	sol = _icp(X, Y, **(dict(x_len=xl, y_len=yl) if N > 1 else {}), max_iterations=ITERS, **kw)
	for n in keep:
		assert sol.status[n].item() == 0 and sol.converged[n].item() and 0 < sol.iterations[n].item() < ITERS, (tag, n, sol.status[n].item(), sol.iterations[n].item())
	sel = torch.tensor(keep)
	for what, t, key in (('R', sol.RTs.R, 'R'), ('t', sol.RTs.T, 't'), ('s', sol.RTs.s, 's')):
		_held(f'{tag} {what}', t.cpu()[sel], _stack([truths[n] for n in keep], key), _stack([r32[n] for n in keep], key), kind='loop ' + what)
	# what is returned belongs to the returned transform: Xt is the fp32 apply, dist / idx its match, rmse their root mean square
	for n in keep:
		p = len(xs[n])
		R, t, s = _tr(sol.RTs, n)
		want = ref.apply(xs[n].astype(np.float64), R, t, s)
		_held(f'{tag} cloud {n} Xt', sol.Xt[n, :p], want, ref.apply(xs[n], R.astype(np.float32), t.astype(np.float32), np.float32(s)), kind='loop Xt')
		used = (sol.dist[n, :p] <= sol.tau[n]).cpu()
		assert int(used.sum()) == sol.used[n].item()
		rmse = math.sqrt(float(sol.dist[n, :p].double().cpu()[used].sum()) / int(used.sum()))
		assert abs(sol.rmse[n].item() - rmse) <= 2 * _ulp(rmse), (tag, n)
	return sol, r64


@pytest.mark.parametrize('P', SIZES)
@pytest.mark.parametrize('N', (1, 3))
def test_rigid_loop_recovers_a_shuffled_copy(P, N):
	xs, ys, truths = _copy_case(P, N, seed=140 + P + N, degrees=12, t_mm=(20, -10, 15), s=1., floor=4)
	sol, _ = _whole_loop(f'rigid loop P={P} N={N}', xs, ys, truths, skip=(2,))
	assert (sol.RTs.s == 1).all()
	if N == 3:   # the cloud of two points: degenerate at once, the identity it started from
		assert sol.status[2].item() == 2 and sol.iterations[2].item() == 0 and torch.equal(sol.RTs.R[2].cpu(), torch.eye(3)) and not sol.RTs.T[2].any()


@pytest.mark.parametrize('P', [p for p in SIZES if p >= 63])
@pytest.mark.parametrize('N', (1, 3))
def test_similarity_loop_recovers_a_shuffled_copy(P, N):
	xs, ys, truths = _copy_case(P, N, seed=90 + P + N, degrees=6, t_mm=(4, -3, 2), s=1.05, floor=63)
	_whole_loop(f'similarity loop P={P} N={N}', xs, ys, truths, skip=(2,), estimate_scale=True)


@pytest.mark.parametrize('P', (257, 1000))
def test_trimmed_loop_ignores_the_shank(P):
	"""X: the base cloud and a quarter as many points in a block above it (the shank above a scan's cut); Y: the moved base alone.  Trimming
	a quarter of the pairs recovers the motion; without it the float64 reference itself does not -- why the option exists."""
	rng = np.random.default_rng(700 + P)
	base = _box(rng, P)
	shank = (rng.random((P // 4, 3)) * np.array([0.08, 0.08, 0.10]) + np.array([0., 0.01, 0.08])).astype(np.float32)
	x = np.concatenate([base, shank])[rng.permutation(P + P // 4)]
	R0, t0, s0 = _truth(rng, 8, (4, -3, 2))
	y = ref.apply(base.astype(np.float64), R0, t0, s0)[rng.permutation(P)].astype(np.float32)
	truth = dict(R=R0, t=t0, s=s0)
	sol, r64 = _whole_loop(f'trimmed loop P={P}', [x], [y], [truth], trim=0.25)
	assert sol.used[0].item() >= ref.keep_count(len(x), 0.25) and sol.tau[0].item() < 1e-12
	plain = ref.icp(x, y, max_iterations=ITERS)
	err = ref.rotation_error(plain['R'], R0)
	print(f'trimmed loop P={P}: untrimmed float64 reference: rotation error {err:.3f} rad, rmse {plain["rmse"]:.2e}; trimmed {ref.rotation_error(r64[0]["R"], R0):.2e} rad')
	assert err > 0.4 and plain["rmse"] > 1e-3


def test_a_row_does_not_depend_on_the_batch():
	xs, ys, _ = _copy_case(257, 3, seed=77, degrees=12, t_mm=(20, -10, 15), s=1., floor=4)
	X, xl = _pad(xs)
	Y, yl = _pad(ys)
	batch = _icp(X, Y, x_len=xl, y_len=yl, max_iterations=ITERS, trim=0.1)
	for n in range(3):
		p = len(xs[n])
		alone = _icp(torch.from_numpy(xs[n])[None], torch.from_numpy(ys[n])[None], max_iterations=ITERS, trim=0.1)
		for a, b in ((alone.RTs.R, batch.RTs.R), (alone.RTs.T, batch.RTs.T), (alone.RTs.s, batch.RTs.s), (alone.rmse, batch.rmse), (alone.tau, batch.tau),
					 (alone.iterations, batch.iterations), (alone.status, batch.status), (alone.used, batch.used)):
			assert torch.equal(a[0], b[n]), n
		assert torch.equal(alone.idx[0], batch.idx[n, :p]) and torch.equal(alone.dist[0], batch.dist[n, :p]) and torch.equal(alone.Xt[0], batch.Xt[n, :p])


# ------------------------------------------------------------------ poison
@contextlib.contextmanager
def poisoned_align(byte):
	"""tests/poison.py's proxy on find_amd.align: every torch.empty of the module comes back filled with `byte`."""
	from find_amd import align as mod
	if byte not in poison.PATTERNS:
		raise ValueError(byte)
	assert mod.torch is torch
	proxy = poison._TorchProxy(byte)
	try:
		mod.torch = proxy
		yield proxy
	finally:
		mod.torch = torch


def test_no_call_reads_or_leaves_unwritten_memory():
	from find_amd import align as mod
	xs, ys, _ = _copy_case(300, 3, seed=61, degrees=12, t_mm=(20, -10, 15), s=1., floor=4)
	X, xl = _pad(xs)
	Y, yl = _pad(ys)
	fx, fy, _, FX, FY, FW, flens = _fit_case(257, 3, 'similarity', True, seed=62)[:7]
	P2 = Y.shape[1]

	def run():
		out = {}
		for tag, kw in (('plain', {}), ('trimmed', dict(trim=0.2, estimate_scale=True, max_distance=0.2)), ('one step', dict(max_iterations=1))):
			sol = mod.iterative_closest_point(X.cuda(), Y.cuda(), xl.cuda(), yl.cuda(), max_iterations=kw.pop('max_iterations', 12), **kw)
			for k, t in zip(sol._fields, sol):
				if k == 'RTs':
					out.update({f'{tag} {a}': b.clone() for a, b in zip('RTs', t)})
				else:
					out[f'{tag} {k}'] = (t.to(torch.int32) if t.dtype == torch.bool else t).clone()
		tr, status = mod.corresponding_points_alignment(FX.cuda(), FY.cuda(), FW.cuda(), estimate_scale=True, lengths=flens.cuda(), return_status=True)
		out.update({f'fit {a}': b.clone() for a, b in zip('RTs', tr)}, **{'fit status': status.clone()})
		return out
	runs = []
	for byte in (None, 0xFF, 0x00):
		run()   # (what a forgotten region would hold: the right values of this call)
		with (poisoned_align(byte) if byte is not None else contextlib.nullcontext()) as proxy:
			runs.append(run())
			assert byte is None or proxy.calls == 3 * 12 + 5
	assert mod.torch is torch
	rules = {f'{tag} idx': poison.Rule(irange=(0, P2)) for tag in ('plain', 'trimmed', 'one step')}
	bad = poison.compare('align', *runs, rules)
	assert not bad, '\n'.join(bad)
	assert all(torch.isfinite(v).all() for k, v in runs[1].items() if v.is_floating_point() and not k.endswith('tau'))


# ------------------------------------------------------------------ the stack
def _moved_template(n_verts, N, seed):
	from find_amd import synthetic
	rng = np.random.default_rng(seed)
	v, f = synthetic.template(n_verts)
	truths = [_truth(rng, 6, 4 * rng.normal(size=3), 1.02 + 0.02 * n) for n in range(N)]
	scans = torch.stack([torch.from_numpy(ref.apply(v.double().numpy(), *tr).astype(np.float32)) for tr in truths])
	return v, f, scans, truths


def test_init_registration_gives_the_registration_stage_its_start():
	"""The template moved by a known similarity as the scan: the written rows of reg, through FN.register_points, land the template where the
	float64 reference ICP on the very same samples lands it, to the loop tests' bound -- and near the scan."""
	from find_amd import align, synthetic
	from find_amd import functional as FN
	from find_amd.losses import sample_points_from_meshes
	from find_amd.structures import Meshes
	N, S = 2, 500
	model = synthetic.make_model(1002, train_size=4, val_size=N)
	v, f, scans, truths = _moved_template(1002, N, seed=3)
	batch = dict(mesh=Meshes(scans.cuda(), f.cuda()), idx=torch.arange(N))
	before = model.reg.data.clone()
	sol = align.init_registration(model, batch, val=True, samples=S, generator=torch.Generator(device='cuda').manual_seed(5), max_iterations=ITERS)
	assert torch.equal(model.reg.data, before) and model.reg_val.data.requires_grad   # only reg_val's rows were written, in place
	reg = model.reg_val.data.detach()
	assert torch.isfinite(reg).all() and (reg[:, 6] == reg[:, 7]).all() and (reg[:, 6] == reg[:, 8]).all()
	# the samples it drew, drawn again
	g = torch.Generator(device='cuda').manual_seed(5)
	tv = model.template_verts.data.expand(N, -1, -1).contiguous()
	xs = sample_points_from_meshes(Meshes(tv, f.cuda()), num_samples=S, generator=g).cpu().numpy()
	ys = sample_points_from_meshes(batch['mesh'], num_samples=S, generator=g).cpu().numpy()
	kw = dict(max_iterations=ITERS, trim=0.2, estimate_scale=True)
	r64 = [ref.icp(x, y, dtype=np.float64, **kw) for x, y in zip(xs, ys)]
	r32 = [ref.icp(x, y, dtype=np.float32, **kw) for x, y in zip(xs, ys)]
	landed = FN.register_points(tv, torch.zeros_like(tv), reg)
	tv64 = tv.double().cpu().numpy()
	_held('init_registration: the registered template', landed, np.stack([ref.apply(tv64[n], r64[n]['R'], r64[n]['t'], r64[n]['s']) for n in range(N)]),
		  np.stack([ref.apply(tv64[n].astype(np.float32), r32[n]['R'], r32[n]['t'], r32[n]['s']) for n in range(N)]), kind='init_registration')
	# near the scan: every vertex within the spacing of the samples, sqrt(area / S) -- what point-to-point ICP between two different samplings
	# of one surface can leave -- from 6 degrees and several mm off
	tri = tv[0][f.cuda()].double()
	area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1).sum().item()
	spacing = math.sqrt(area / S)
	off = (landed - scans.cuda()).norm(dim=-1).max().item()
	start = (tv - scans.cuda()).norm(dim=-1).max().item()
	print(f'init_registration: the template lands within {off * 1e3:.2f} mm of the scan (identity: {start * 1e3:.2f} mm; sample spacing {spacing * 1e3:.2f} mm); '
		  f'iterations {sol.iterations.tolist()}')
	assert off < spacing < start
	assert torch.equal(align.reg_from_transform(sol.RTs), reg)


def test_eval_3d_metrics_reports_aligned_errors():
	from find_amd import eval_metrics, synthetic
	from find_amd.structures import Meshes
	v, f = synthetic.template(1002)
	rng = np.random.default_rng(12)
	N, S = 2, 2000
	scan = torch.stack([v * torch.tensor([1.0 + 0.05 * n, 1., 1.]) for n in range(N)])
	moves = [_truth(rng, 5, 5 * rng.normal(size=3)) for _ in range(N)]
	pred = torch.stack([torch.from_numpy(ref.apply(scan[n].double().numpy(), *moves[n]).astype(np.float32)) for n in range(N)])
	gt_m, same_m, pred_m = Meshes(scan.cuda(), f.cuda()), Meshes(scan.clone().cuda(), f.cuda()), Meshes(pred.cuda(), f.cuda())
	kp = [3, 17, 40, 101]
	kw = dict(template_kp_idxs=kp, gt_kps=scan[:, kp].cuda(), samples=S)

	def call(pm, pv, **more):
		torch.manual_seed(21)
		return eval_metrics.eval_3d_metrics(pm, gt_m, pred_verts=pv.cuda(), **kw, **more)
	unmoved = call(same_m, scan)
	plain = call(pred_m, pred)
	out, per_foot = call(pred_m, pred, align='rigid', return_per_foot=True)
	assert list(out) == list(plain) + ['Chamf aligned (μm)', 'Keypoint aligned (mm)'] and all(torch.equal(out[k], plain[k]) for k in plain)   # the same draws
	assert list(per_foot) == ['align_R', 'align_T', 'align_s', 'align_rmse'] and (per_foot['align_s'] == 1).all()
	# the moved prediction's samples are the unmoved one's samples, moved (the same draws on a congruent mesh): after alignment the Chamfer
	# term is the unmoved one.  Its size is set by the spacing of the samples; the alignment can be off by what ICP between two different
	# samplings of one surface leaves, which the float64 reference on the same samples measures.
	print(f"Chamf (μm): unmoved {unmoved['Chamf (μm)'].item():.4f}, moved {plain['Chamf (μm)'].item():.4f}, aligned {out['Chamf aligned (μm)'].item():.4f}; "
		  f"keypoints (mm): moved {plain['Keypoint (mm)'].item():.4f}, aligned {out['Keypoint aligned (mm)'].item():.4f}")
	torch.manual_seed(21)
	_, (gt_pts, pred_pts) = eval_metrics.eval_3d_metrics(pred_m, gt_m, samples=S, return_samples=True)
	r64 = [ref.icp(x, y, dtype=np.float64) for x, y in zip(pred_pts.cpu().numpy(), gt_pts.cpu().numpy())]
	r32 = [ref.icp(x, y, dtype=np.float32) for x, y in zip(pred_pts.cpu().numpy(), gt_pts.cpu().numpy())]

	def chamfer(a, b):
		return float(np.mean([ref.nearest(p, q)[0].mean() + ref.nearest(q, p)[0].mean() for p, q in zip(a, b)])) * 1e6
	g64 = gt_pts.double().cpu().numpy()
	c64 = chamfer(g64, [ref.apply(p, r['R'], r['t'], r['s']) for p, r in zip(pred_pts.double().cpu().numpy(), r64)])
	c32 = chamfer(g64.astype(np.float32), [ref.apply(p, r['R'], r['t'], r['s']) for p, r in zip(pred_pts.cpu().numpy(), r32)])
	_held('Chamf aligned (μm)', out['Chamf aligned (μm)'].reshape(1), [c64], [c32], kind='Chamf aligned')
	# against the unmoved value: ICP settles where the two SAMPLED clouds fit best, which is not exactly the motion that was applied (the float64
	# reference lands in the same place, as the line above holds), so the aligned term equals the unmoved one only to the few per cent by which
	# two samplings of one surface can be slid into each other -- not to rounding.  It must undo the motion's share of the error, though.
	gap = abs(c64 - unmoved['Chamf (μm)'].item()) / unmoved['Chamf (μm)'].item()
	print(f'Chamf aligned: float64 reference {c64:.4f}, {100 * gap:.2f} % from the unmoved value')
	assert abs(out['Chamf aligned (μm)'].item() - unmoved['Chamf (μm)'].item()) <= 0.1 * unmoved['Chamf (μm)'].item() and out['Chamf aligned (μm)'] < plain['Chamf (μm)']
	kp64 = np.stack([ref.apply(pred[n, kp].double().numpy(), r['R'], r['t'], r['s']) for n, r in enumerate(r64)])
	kp32 = np.stack([ref.apply(pred[n, kp].numpy(), r['R'], r['t'], r['s']) for n, r in enumerate(r32)])
	err64, err32 = (np.linalg.norm(k.astype(np.float64) - scan[:, kp].double().numpy(), axis=-1).mean() * 1e3 for k in (kp64, kp32))
	_held('Keypoint aligned (mm)', out['Keypoint aligned (mm)'].reshape(1), [err64], [err32], kind='Keypoint aligned')
	assert out['Keypoint aligned (mm)'] < plain['Keypoint (mm)']
	sim = call(pred_m, pred, align='similarity')
	assert list(sim) == list(out) and torch.isfinite(sim['Chamf aligned (μm)'])


def test_eval_3d_passes_align_through(tmp_path):
	"""evaluate.eval_3d(align=...) on the four keypointed synthetic scans of tests/test_gpu_points.py: the two keys beside today's numbers,
	the per-foot transforms, and exactly today's dict without the keyword."""
	from tests.test_gpu_eval2d import _model
	from tests.test_gpu_points import _foot3d_val_kp
	from find_amd import evaluate
	ds = _foot3d_val_kp(tmp_path)
	model = _model(len(ds))
	kp_idx = [3, 17, 40, 101]
	torch.manual_seed(31)
	plain = evaluate.eval_3d(model, ds, kp_idx, samples=500)
	torch.manual_seed(31)
	none = evaluate.eval_3d(model, ds, kp_idx, samples=500, align=None)
	torch.manual_seed(31)
	res, extra = evaluate.eval_3d(model, ds, kp_idx, samples=500, return_per_foot=True, align='similarity')
	new = ['Chamf aligned (μm)', 'Keypoint aligned (mm)']
	assert list(plain) == ['Keypoint (mm)', 'Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)'] and none == plain
	assert list(res) == list(plain) + new and all(res[k] == plain[k] for k in plain)   # no draw was added
	assert all(isinstance(res[k], float) and np.isfinite(res[k]) and res[k] > 0 for k in new)
	assert list(extra) == ['keypoint_mm', 'align_R', 'align_T', 'align_s', 'align_rmse']
	assert extra['align_R'].shape == (4, 3, 3) and extra['align_T'].shape == (4, 3) and extra['align_s'].shape == extra['align_rmse'].shape == (4,)
	assert all(torch.isfinite(extra[k]).all() for k in extra) and res['Chamf aligned (μm)'] <= res['Chamf (μm)']
	torch.manual_seed(31)
	rigid = evaluate.eval_3d(model, ds, kp_idx, samples=500, align='rigid')
	assert list(rigid) == list(res) and rigid['Chamf (μm)'] == plain['Chamf (μm)']


def test_print_the_worst_ratios():
	"""Not a check of its own: the worst e_hip / max(e32, ulp) of the comparisons above, per quantity, for the test log."""
	print('worst e_hip / max(e32, 1 ulp) per quantity:', {k: round(v, 3) for k, v in WORST.items()})
