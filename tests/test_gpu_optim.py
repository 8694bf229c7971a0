"""Fused optimisers (C-ABI find_adam_step / find_sgd_step behind find_amd.optim) against the oracle's golden trajectories and
against torch.optim running on the same device: the three optimisers of the reference's step (train.py:161-168)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import optim_f64_ref as R
from tests.test_oracle_optim import CASES, GOLD, SHAPES, STEPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
	return np.load(GOLD)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_step_matches_golden_trajectory(gold, name):
	from find_amd import optim
	kind, kw = CASES[name]
	ps = [torch.nn.Parameter(torch.from_numpy(gold[f'p0/{i}']).cuda()) for i in range(SHAPES)]
	opt = (optim.Adam if kind == 'adam' else optim.SGD)(ps, **kw)
	for k in range(STEPS):
		for i, p in enumerate(ps):
			p.grad = torch.from_numpy(gold[f'grad/{k}/{i}']).cuda()
		opt.step()
		for i, p in enumerate(ps):
			ref = gold[f'{name}/{k}/{i}']
			assert np.allclose(p.detach().cpu().numpy(), ref, rtol=2e-6, atol=1e-7), (name, k, i)


def test_find_parameter_set_matches_torch_optim_and_state_dict_is_compatible():
	"""The real parameter set (MLP + latent tables + registration, 16 training feet): 5 steps of the reference's three optimisers,
	fused vs torch.optim on the same GPU; the state_dict of one loads into the other."""
	from find_amd import optim, synthetic
	g = torch.Generator().manual_seed(0)
	models = [synthetic.make_model(1002, train_size=16, val_size=2, device='cuda') for _ in range(2)]
	models[1].load_state_dict(models[0].state_dict())

	def groups(m):
		return [p for p in m.main_params], [p for p in m.reg_params], [p for p in m.latent_params]

	(n0, r0, l0), (n1, r1, l1) = groups(models[0]), groups(models[1])
	fused = [optim.Adam(n0, lr=5e-4), optim.SGD(r0, lr=1e-2, momentum=0.9), optim.Adam(l0, lr=1e-3)]
	ref = [torch.optim.Adam(n1, lr=5e-4), torch.optim.SGD(r1, lr=1e-2, momentum=0.9), torch.optim.Adam(l1, lr=1e-3)]
	for k in range(5):
		for pa, pb in zip(n0 + r0 + l0, n1 + r1 + l1):
			gr = torch.randn(pa.shape, generator=g).cuda() * 0.1
			pa.grad, pb.grad = gr.clone(), gr.clone()
		for o in fused + ref:
			o.step()
	for pa, pb in zip(n0 + r0 + l0, n1 + r1 + l1):
		assert torch.allclose(pa, pb, rtol=2e-6, atol=1e-7)
	# state round trip: torch's optimiser continues from the fused one's state and vice versa
	sd = fused[0].state_dict()
	t2 = torch.optim.Adam(n1, lr=5e-4)
	t2.load_state_dict(sd)
	f2 = optim.Adam(n0, lr=5e-4)
	f2.load_state_dict(ref[0].state_dict())
	for pa, pb in zip(n0, n1):
		gr = torch.randn(pa.shape, generator=g).cuda() * 0.1
		pa.grad, pb.grad = gr.clone(), gr.clone()
	f2.step(); t2.step()
	for pa, pb in zip(n0, n1):
		assert torch.allclose(pa, pb, rtol=4e-6, atol=2e-7)


def test_optimiser_rejects_cpu_parameters():
	from find_amd import optim
	p = torch.nn.Parameter(torch.zeros(4))
	p.grad = torch.ones(4)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		optim.Adam([p]).step()


def test_adam_capturable_matches_default_path():
	"""Adam(capturable=True): step count on the device, bias corrections formed there in fp32 (find_adam_step_dev) -- the same
	trajectory as the default host-arithmetic path to fp32 rounding, and the same state_dict layout."""
	from find_amd import optim
	g = torch.Generator().manual_seed(3)
	shapes = [(256, 515), (256,), (7, 100), (3, 256)]
	init = [torch.randn(*s, generator=g) for s in shapes]
	grads = [[torch.randn(*s, generator=g) * 0.1 for s in shapes] for _ in range(8)]
	res = []
	for cap in (False, True):
		ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
		opt = optim.Adam(ps, lr=5e-4, weight_decay=1e-3, capturable=cap)
		for gs in grads:
			for p, gr in zip(ps, gs):
				p.grad = gr.cuda()
			opt.step()
		torch.cuda.synchronize()
		res.append((ps, opt))
	(pa, oa), (pb, ob) = res
	for a, b in zip(pa, pb):
		assert (a - b).abs().max().item() < 1e-6 * max(1.0, a.abs().max().item())
	sa, sb = oa.state_dict(), ob.state_dict()
	assert sa['state'].keys() == sb['state'].keys()
	for k in sa['state']:
		assert set(sa['state'][k]) == set(sb['state'][k]) == {'step', 'exp_avg', 'exp_avg_sq'}
		assert float(sa['state'][k]['step']) == float(sb['state'][k]['step']) == 8.0
		assert sb['state'][k]['step'].is_cuda and not sa['state'][k]['step'].is_cuda
		assert torch.allclose(sa['state'][k]['exp_avg_sq'], sb['state'][k]['exp_avg_sq'])
	# the capturable optimiser keeps one counter per bucket inside; a state_dict holds a copy per parameter (no aliasing, no later movement)
	steps = [sb['state'][k]['step'] for k in sb['state']]
	assert len({t.data_ptr() for t in steps}) == len(steps)
	for p, gr in zip(pb, grads[0]):
		p.grad = gr.cuda()
	ob.step()
	torch.cuda.synchronize()
	assert all(float(t) == 8.0 for t in steps) and float(ob.state_dict()['state'][0]['step']) == 9.0
	# ... and loads back into a fresh optimiser that continues the same trajectory
	ps2 = [torch.nn.Parameter(t.detach().clone()) for t in pb]
	o2 = optim.Adam(ps2, lr=5e-4, weight_decay=1e-3, capturable=True)
	import copy
	o2.load_state_dict(copy.deepcopy(ob.state_dict()))   # (torch's load_state_dict keeps tensors that already have the right dtype and device: the moments would be shared)
	for q, p, gr in zip(ps2, pb, grads[1]):
		q.grad = gr.cuda(); p.grad = gr.cuda()
	o2.step(); ob.step()
	torch.cuda.synchronize()
	for q, p in zip(ps2, pb):
		assert torch.equal(q, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# The update itself, in units: every test below measures |fp32 result - float64 restatement| / unit per entry (tests/optim_f64_ref.py)
# for the fused op and for torch.optim(foreach=False, fused=False) on the same GPU, and asserts fused <= 2 x torch for the parameter and
# every moment: both are legitimate fp32 evaluation orders of one formula that differ in FMA contraction.  The fused op is never its own
# reference.  States (a step count, given moments) are placed by load_state_dict, not by stepping.
# Adam(capturable=True) (find_adam_step_dev) is not among the cases yet: that path is unchanged, still forms 1 - beta in fp32 and refuses
# 0-element tensors, and would miss the unit rule; the helpers keep their `capturable` argument for the day it follows.
# ---------------------------------------------------------------------------------------------------------------------------------
DEV = 'cuda'
LR = 3e-3          # lr, betas, eps and weight_decay are pairwise distinct in every case: a swapped C argument shows
ADAM_GRID = list(itertools.product((1, 2, 10, 1000, 100000), ((0.9, 0.999), (0.8, 0.99), (0.0, 0.5)), (1e-8, 1e-6, 1e-3), (0.0, 0.01))) \
	+ list(itertools.product((1, 1000), ((0.9, 0.999), (0.8, 0.99), (0.0, 0.5)), (0.0,), (0.0, 0.01)))
SGD_GRID = [(mu, d, wd, nes) for mu, d, wd, nes in itertools.product((0.0, 0.9), (0.0, 0.3), (0.0, 0.05), (False, True))
			if not (nes and (mu == 0 or d != 0))]


def _t(a):
	return torch.from_numpy(np.array(a, order='C')).to(DEV)       # (a copy: never the caller's memory)


def _n(t):
	return None if t is None else t.detach().cpu().numpy()


def _bits(t):
	return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _make(kind, fused, params, **kw):
	from find_amd import optim
	if fused:
		return (optim.Adam if kind == 'adam' else optim.SGD)(params, **kw)
	return (torch.optim.Adam if kind == 'adam' else torch.optim.SGD)(params, foreach=False, fused=False, **kw)


def _load(opt, states):
	"""states[i]: the state dict of the i-th parameter (in param_groups order), or None for no state."""
	sd = opt.state_dict()
	sd['state'] = {i: s for i, s in enumerate(states) if s is not None}
	opt.load_state_dict(sd)


def _adam_state(step, m, v):
	return dict(step=torch.tensor(float(step)), exp_avg=m.clone(), exp_avg_sq=v.clone())


def _report(label, worst):
	print(f'[optim-units] {label}: ' + ' | '.join(f'{who} ' + ' '.join(f'{q}={x:.3g}' for q, x in w.items()) for who, w in worst.items()))


def _hold(label, got_fused, got_torch, want, units, worst, cap=False):
	"""One case: the unit rule for each quantity; NaN positions equal torch's and the restatement's.  cap: torch.optim itself within HOST_CAP."""
	for q in want:
		f, t, w, u = got_fused[q], got_torch[q], want[q], units[q]
		assert np.array_equal(np.isnan(f), np.isnan(t)) and np.array_equal(np.isnan(t), np.isnan(w)), (label, q)
		wf, wt = R.worst(f, w, u), R.worst(t, w, u)
		worst['fused'][q] = max(worst['fused'].get(q, 0.0), wf)
		worst['torch'][q] = max(worst['torch'].get(q, 0.0), wt)
		assert wf <= 2.0 * wt, (label, q, wf, wt)
		if cap:
			assert wt <= R.HOST_CAP[q], (label, q, wt)


@pytest.fixture(scope='module')
def gen():
	arrs = R.make_inputs(20_000, seed=1)
	return arrs, tuple(_t(a) for a in arrs)


def _adam_once(fused, dev_in, step, betas, eps, wd, capturable):
	p0, g, m0, v0 = dev_in
	p = torch.nn.Parameter(p0.clone())
	p.grad = g.clone()
	opt = _make('adam', fused, [p], lr=LR, betas=betas, eps=eps, weight_decay=wd, capturable=capturable)
	_load(opt, [_adam_state(step - 1, m0, v0)])
	opt.step()
	st = opt.state[p]
	assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))      # weight decay does not write the gradient
	assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
	return dict(p=_n(p), m=_n(st['exp_avg']), v=_n(st['exp_avg_sq'])), st['step']


def _adam_grid(gen, capturable):
	arrs, dev_in = gen
	worst = dict(fused={}, torch={})
	for step, betas, eps, wd in ADAM_GRID:
		label = f'adam capturable={capturable} step={step} betas={betas} eps={eps} wd={wd}'
		with np.errstate(invalid='ignore', divide='ignore'):
			(P, M, V), (up, um, uv) = R.adam_step(*arrs, step, lr=LR, betas=betas, eps=eps, weight_decay=wd)
		gf, sf = _adam_once(True, dev_in, step, betas, eps, wd, capturable)
		gt, stt = _adam_once(False, dev_in, step, betas, eps, wd, capturable)
		assert torch.is_tensor(sf) and sf.dtype == torch.float32 and sf.is_cuda == capturable == stt.is_cuda and float(sf) == float(stt) == float(step), label
		_hold(label, gf, gt, dict(p=P, m=M, v=V), dict(p=up, m=um, v=uv), worst, cap=not capturable)
		if eps == 0 and wd == 0:
			assert np.isnan(gf['p']).sum() == len(range(0, len(P), 97)), label
	_report(f'adam one step, {"capturable" if capturable else "host"} path, {len(ADAM_GRID)} cases x {len(arrs[0])}', worst)


def test_adam_host_path_one_step_in_units(gen):
	"""find_adam_step over steps x betas x eps x weight decay (and eps = 0: NaN exactly where torch has it) against torch.optim.Adam."""
	_adam_grid(gen, False)


def test_sgd_first_and_second_step_in_units(gen):
	"""The first step clones the (decayed) gradient, dampening ignored; the second dampens.  Without momentum no buffer is made."""
	arrs, dev_in = gen
	p0, g, m0, _ = dev_in
	worst = dict(fused={}, torch={})
	for (mu, d, wd, nes), first in itertools.product(SGD_GRID, (True, False)):
		label = f'sgd first={first} momentum={mu} dampening={d} wd={wd} nesterov={nes}'
		buf0 = None if (first or mu == 0) else arrs[2]
		(P, B), (up, ub) = R.sgd_step(arrs[0], arrs[1], buf0, LR, mu, d, wd, nes)
		got = []
		for fused in (True, False):
			p = torch.nn.Parameter(p0.clone())
			p.grad = g.clone()
			opt = _make('sgd', fused, [p], lr=LR, momentum=mu, dampening=d, weight_decay=wd, nesterov=nes)
			if buf0 is not None:
				_load(opt, [dict(momentum_buffer=m0.clone())])
			opt.step()
			assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))
			assert ('momentum_buffer' in opt.state[p]) == (mu != 0), label
			got.append(dict(p=_n(p), buf=_n(opt.state[p]['momentum_buffer'])) if mu != 0 else dict(p=_n(p)))
		want, units = (dict(p=P, buf=B), dict(p=up, buf=ub)) if mu != 0 else (dict(p=P), dict(p=up))
		_hold(label, got[0], got[1], want, units, worst, cap=True)
	_report(f'sgd first and second step, {2 * len(SGD_GRID)} cases x {len(arrs[0])}', worst)


# ---- launch geometry ------------------------------------------------------------------------------------------------------------
SENT = 3                       # sentinel floats between neighbouring tensors of an arena (odd: it also de-aligns them)
SENT_BITS = 0x7FC0DEAD         # a quiet NaN with a payload


def _cuts(n):
	edges = [1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]
	rng = np.random.default_rng(5)
	cuts = {'one': [n], 'edges': edges + [n - sum(edges)]}
	for name, empty in (('97 with empties', (0, 47, 48, 60, 96)), ('97 ending full', (0, 60))):
		w = 10.0 ** rng.uniform(0.0, 3.0, 97)
		w[list(empty)] = 0.0
		sizes = np.floor(w / w.sum() * (n - 97)).astype(int) + (w > 0)
		sizes[1] += n - sizes.sum()
		assert sizes.sum() == n and all(sizes[i] == 0 for i in empty) and (sizes > 0).sum() == 97 - len(empty) and sizes.max() > 2048
		cuts[name] = [int(s) for s in sizes]
	return cuts


def _arena(flat, sizes):
	"""flat (fp32 numpy) laid out as len(sizes) tensors with SENT sentinels before, between and after; returns the device arena, its views, and
	the boolean mask of the sentinels."""
	total = sum(sizes) + SENT * (len(sizes) + 1)
	host = np.full(total, SENT_BITS, dtype=np.uint32).view(np.float32)
	mask = np.ones(total, dtype=bool)
	offs, o, src = [], SENT, 0
	for s in sizes:
		host[o:o + s] = flat[src:src + s]
		mask[o:o + s] = False
		offs.append(o)
		o += s + SENT
		src += s
	dev = _t(host)
	return dev, [dev[o:o + s] for o, s in zip(offs, sizes)], mask


def _geometry_run(kind, arrs, sizes, capturable=False, first=False):
	"""One fused step of the flat vector cut into `sizes`; returns the bits of p and of the moments, tensor after tensor, flat."""
	p0, g0, m0, v0 = arrs
	(ap, vp, mask), (ag, vg, _), (am, vm, _), (av, vv, _) = (_arena(a, sizes) for a in (p0, g0, m0, v0))
	g_before = _bits(ag)
	ps = [torch.nn.Parameter(v) for v in vp]
	for p, v, gr in zip(ps, vp, vg):
		assert p.data_ptr() == v.data_ptr()
		p.grad = gr
	if kind == 'adam':
		opt = _make('adam', True, ps, lr=LR, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01, capturable=capturable)
		for p, m, v in zip(ps, vm, vv):
			opt.state[p] = dict(step=torch.tensor(7.0, device=DEV if capturable else 'cpu'), exp_avg=m, exp_avg_sq=v)
	else:
		opt = _make('sgd', True, ps, lr=LR, momentum=0.9, dampening=0.3, weight_decay=0.05)
		if not first:
			for p, m in zip(ps, vm):
				opt.state[p] = dict(momentum_buffer=m)
	opt.step()
	torch.cuda.synchronize()
	assert np.array_equal(_bits(ag), g_before), 'the gradient arena was written'
	arenas = [ap] if (kind == 'sgd' and first) else [ap, am] if kind == 'sgd' else [ap, am, av]
	for a in arenas:
		assert np.all(_bits(a)[mask] == np.int32(SENT_BITS)), 'a sentinel between two tensors was written'
	out = [_bits(a)[~mask] for a in arenas]
	if kind == 'sgd' and first:
		bufs = [opt.state[p]['momentum_buffer'] for p in ps]
		assert all(b.shape == p.shape for b, p in zip(bufs, ps))
		out.append(np.concatenate([_bits(b) for b in bufs]))
	if kind == 'adam':
		assert all(float(opt.state[p]['step']) == 8.0 for p in ps)
	return out


@pytest.mark.parametrize('kind,capturable,first', [('adam', False, False), ('sgd', False, True), ('sgd', False, False)])
def test_launch_geometry_is_bit_exact(kind, capturable, first):
	"""The op is elementwise: one vector stepped as one tensor, cut at the CHUNK = 2048 edges, and cut into 97 tensors (two launches of 48 and a
	third, 0-element tensors first, at 47 | 48, inside and last) gives identical bits; nothing between the tensors and no gradient is written."""
	n = 40_000
	arrs = R.make_inputs(n, seed=2)
	ref = None
	for name, sizes in _cuts(n).items():
		out = _geometry_run(kind, arrs, sizes, capturable=capturable, first=first)
		if ref is None:
			ref = out
			continue
		for a, b in zip(ref, out):
			assert np.array_equal(a, b), (kind, capturable, first, name)


@pytest.mark.parametrize('kind,kw', [('adam', dict()), ('sgd', dict(momentum=0.9))])
def test_empty_parameter_steps_as_in_torch(kind, kw):
	"""A 0-element device tensor has data_ptr() == 0; torch.optim steps it without complaint, and so does the fused step (the C-ABI accepts NULL
	where numel == 0)."""
	states = []
	for fused in (True, False):
		p = torch.nn.Parameter(torch.empty(0, device=DEV))
		p.grad = torch.empty(0, device=DEV)
		opt = _make(kind, fused, [p], lr=LR, **kw)
		opt.step(); opt.step()
		torch.cuda.synchronize()
		states.append(opt.state[p])
	a, b = states
	assert set(a) == set(b)
	for k in a:
		assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].device == b[k].device, k
	if kind == 'adam':
		assert float(a['step']) == float(b['step']) == 2.0


def test_row_with_zero_gradient_still_moves():
	"""Dense Adam over a latent table: rows whose gradient is exactly 0 move with their moments (and the moments decay), as the float64
	restatement says."""
	rng = np.random.default_rng(11)
	shape, rows = (16, 100), [0, 7, 15]
	p0 = rng.standard_normal(shape).astype(np.float32)
	g = (rng.standard_normal(shape) * 0.1).astype(np.float32)
	g[rows] = 0.0
	m0 = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.01, 0.1, shape)).astype(np.float32)
	v0 = (rng.uniform(1e-4, 1e-2, shape)).astype(np.float32)
	(P, M, V), (up, um, uv) = R.adam_step(p0, g, m0, v0, 4, lr=LR)
	got = []
	for fused in (True, False):
		p = torch.nn.Parameter(_t(p0))
		p.grad = _t(g)
		opt = _make('adam', fused, [p], lr=LR)
		_load(opt, [_adam_state(3, _t(m0), _t(v0))])
		opt.step()
		got.append(dict(p=_n(p)[rows], m=_n(opt.state[p]['exp_avg'])[rows], v=_n(opt.state[p]['exp_avg_sq'])[rows]))
	worst = dict(fused={}, torch={})
	_hold('zero rows', got[0], got[1], dict(p=P[rows], m=M[rows], v=V[rows]), dict(p=up[rows], m=um[rows], v=uv[rows]), worst, cap=True)
	assert np.all(got[0]['p'] != p0[rows]) and np.all(np.abs(got[0]['m']) < np.abs(m0[rows])) and np.all(got[0]['v'] < v0[rows])
	_report('adam, rows with zero gradient', worst)


# ---- trajectories: groups, buckets, schedules ---------------------------------------------------------------------------------
def _run(kind, fused, groups, p0s, grads, states=None, sched=False, keep=None):
	"""groups: list of (indices, keywords).  grads[k][i]: numpy or None.  Returns the history [step][param] -> dict(p, m, v | buf) of device
	clones (None where a parameter has no state yet) and the optimiser."""
	ps = [torch.nn.Parameter(_t(a)) for a in p0s]
	if keep is not None:
		keep.extend(ps)
	opt = _make(kind, fused, [dict(params=[ps[i] for i in idx], **kw) for idx, kw in groups])
	order = [i for idx, _ in groups for i in idx]
	if states is not None:
		_load(opt, [states[i] for i in order])
	sch = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5) if sched else None
	hist = []
	for gs in grads:
		for p, gr in zip(ps, gs):
			p.grad = None if gr is None else (gr if torch.is_tensor(gr) else _t(gr))
		opt.step()
		if sch is not None:
			sch.step()
		row = []
		for p in ps:
			st = opt.state.get(p, {})
			e = dict(p=p.detach().clone())
			if kind == 'adam':
				e['m'] = st['exp_avg'].clone() if 'exp_avg' in st else None
				e['v'] = st['exp_avg_sq'].clone() if 'exp_avg_sq' in st else None
			elif st.get('momentum_buffer') is not None:
				e['buf'] = st['momentum_buffer'].clone()
			row.append(e)
		hist.append(row)
	return hist, opt, ps


def _f64_run(kind, hps, p0s, grads, states=None, gamma=1.0):
	"""The float64 trajectory of every parameter fed the same gradients, with the units summed over the steps it has taken.
	hps[i]: keywords of parameter i.  Returns [step][param] -> (values, summed units)."""
	cur = []
	for i, p0 in enumerate(p0s):
		st = (states[i] if states is not None else None) or {}
		if kind == 'adam':
			cur.append(dict(p=np.asarray(p0, np.float64), m=_n(st['exp_avg']) if st else np.zeros(p0.shape), v=_n(st['exp_avg_sq']) if st else np.zeros(p0.shape),
							step=int(st['step']) if st else 0))
		else:
			cur.append(dict(p=np.asarray(p0, np.float64), buf=_n(st.get('momentum_buffer')) if st else None))
	acc = [dict() for _ in p0s]
	hist = []
	for k, gs in enumerate(grads):
		row = []
		for i, gr in enumerate(gs):
			c, hp = cur[i], dict(hps[i])
			hp['lr'] = hp['lr'] * gamma ** k
			if gr is not None:
				gr = np.ascontiguousarray(_n(gr) if torch.is_tensor(gr) else gr)
				if kind == 'adam':
					c['step'] += 1
					(c['p'], c['m'], c['v']), us = R.adam_step(c['p'], gr, c['m'], c['v'], c['step'], **hp)
					for q, u in zip('pmv', us):
						acc[i][q] = acc[i].get(q, 0.0) + u
				else:
					(c['p'], c['buf']), (u_p, u_b) = R.sgd_step(c['p'], gr, c['buf'], **hp)
					acc[i]['p'] = acc[i].get('p', 0.0) + u_p
					if u_b is not None:
						acc[i]['buf'] = acc[i].get('buf', 0.0) + u_b
			row.append(({q: x for q, x in c.items() if q != 'step' and x is not None}, dict(acc[i])))
		hist.append(row)
	return hist


def _hold_traj(label, hf, ht, h64, worst=None):
	"""Fused <= 2 x torch over the whole trajectory: the worst error in summed units over all steps and parameters, per quantity."""
	worst = dict(fused={}, torch={}) if worst is None else worst
	w = dict(fused={}, torch={})
	for rf, rt, r64 in zip(hf, ht, h64):
		for ef, et, (want, units) in zip(rf, rt, r64):
			for q, x in want.items():
				if q not in units:
					continue          # no step taken yet: nothing to be off by
				assert ef.get(q) is not None and et.get(q) is not None, (label, q)
				w['fused'][q] = max(w['fused'].get(q, 0.0), R.worst(_n(ef[q]), x, units[q]))
				w['torch'][q] = max(w['torch'].get(q, 0.0), R.worst(_n(et[q]), x, units[q]))
	for q in w['torch']:
		assert w['fused'][q] <= 2.0 * w['torch'][q], (label, q, w['fused'][q], w['torch'][q])
		for who in w:
			worst[who][q] = max(worst[who].get(q, 0.0), w[who][q])
	return worst


def _same_bits(ha, hb):
	for ra, rb in zip(ha, hb):
		for ea, eb in zip(ra, rb):
			for q in ea:
				assert (ea[q] is None) == (eb[q] is None) and (ea[q] is None or torch.equal(ea[q].view(torch.int32), eb[q].view(torch.int32))), q


def _draws(seed, shapes, steps):
	"""Initial parameters, previous moments and `steps` gradients per tensor from the generator (gradients do not depend on the parameters)."""
	out = []
	for j, s in enumerate(shapes):
		n = int(np.prod(s))
		p, g, m, v = R.make_inputs(n, seed=seed + 100 * j)
		gs = [g] + [R.make_inputs(n, seed=seed + 100 * j + k)[1] for k in range(1, steps)]
		out.append((p.reshape(s), [x.reshape(s) for x in gs], m.reshape(s), v.reshape(s)))
	return out


ADAM_A = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
ADAM_B = dict(lr=7e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
SGD_A = dict(lr=LR, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
SGD_B = dict(lr=7e-4, momentum=0.8, dampening=0.3, weight_decay=0.05, nesterov=False)


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_two_param_groups_equal_two_optimisers(kind):
	d = _draws(20, [(3000,), (2049,), (17, 5)], 3)
	p0s = [x[0] for x in d]
	grads = [[x[1][k] for x in d] for k in range(3)]
	A, B = (ADAM_A, ADAM_B) if kind == 'adam' else (SGD_A, SGD_B)
	groups = [([0, 2], A), ([1], B)]
	hf, _, _ = _run(kind, True, groups, p0s, grads)
	ht, _, _ = _run(kind, False, groups, p0s, grads)
	h64 = _f64_run(kind, [A, B, A], p0s, grads)
	_report(f'{kind}, two param groups, 3 steps', _hold_traj('two groups', hf, ht, h64))
	# ... and one optimiser per group gives the same bits
	ha, _, _ = _run(kind, True, [([0, 1], A)], [p0s[0], p0s[2]], [[gs[0], gs[2]] for gs in grads])
	hb, _, _ = _run(kind, True, [([0], B)], [p0s[1]], [[gs[1]] for gs in grads])
	_same_bits(hf, [[ra[0], rb[0], ra[1]] for ra, rb in zip(ha, hb)])


@pytest.mark.parametrize('capturable', [False])
def test_adam_parameters_at_different_step_counts(capturable):
	"""One group, parameters at step counts 0 (no state), 3 and 1000: three buckets, each with its own bias corrections."""
	d = _draws(30, [(2500,), (2048,), (33, 9)], 3)
	p0s = [x[0] for x in d]
	grads = [[x[1][k] for x in d] for k in range(3)]
	hp = dict(ADAM_B, capturable=capturable)
	mk = lambda: [None, _adam_state(3, _t(d[1][2]), _t(d[1][3])), _adam_state(1000, _t(d[2][2]), _t(d[2][3]))]
	hf, of, pf = _run('adam', True, [([0, 1, 2], hp)], p0s, grads, states=mk())
	ht, ot, pt = _run('adam', False, [([0, 1, 2], hp)], p0s, grads, states=mk())
	for a, b, want in zip(pf, pt, (3.0, 6.0, 1003.0)):
		sa, sb = of.state[a]['step'], ot.state[b]['step']
		assert float(sa) == float(sb) == want and sa.is_cuda == sb.is_cuda == capturable
	h64 = _f64_run('adam', [ADAM_B] * 3, p0s, grads, states=mk())
	_report(f'adam capturable={capturable}, step counts 0 / 3 / 1000, 3 steps', _hold_traj('buckets', hf, ht, h64))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_parameter_whose_gradient_appears_late(kind):
	"""A parameter without a gradient for two steps: Adam re-buckets when it joins (step 1 beside step 3), SGD takes the clone-the-gradient first
	step for it and the momentum step for the other in one call."""
	d = _draws(40, [(2100,), (1500,)], 4)
	p0s = [x[0] for x in d]
	grads = [[d[0][1][k], d[1][1][k] if k >= 2 else None] for k in range(4)]
	hp = ADAM_B if kind == 'adam' else SGD_B
	hf, of, pf = _run(kind, True, [([0, 1], hp)], p0s, grads)
	ht, ot, pt = _run(kind, False, [([0, 1], hp)], p0s, grads)
	assert torch.equal(hf[1][1]['p'], _t(p0s[1])) and len(of.state[pf[1]]) == len(ot.state[pt[1]])
	if kind == 'adam':
		assert [float(of.state[p]['step']) for p in pf] == [float(ot.state[p]['step']) for p in pt] == [4.0, 2.0]
	h64 = _f64_run(kind, [hp, hp], p0s, grads)
	_report(f'{kind}, gradient appears at the third step, 4 steps', _hold_traj('late gradient', hf, ht, h64))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_transposed_gradient_and_step_lr(kind):
	"""A non-contiguous (transposed) gradient, and lr halved after every step by torch.optim.lr_scheduler.StepLR."""
	d = _draws(50, [(53, 37), (2049,)], 3)
	p0s = [d[0][0].T.copy(), d[1][0]]                                   # parameter 0 is (37, 53); its gradients arrive as views of (53, 37)
	grads = [[_t(d[0][1][k]).t(), d[1][1][k]] for k in range(3)]
	assert not grads[0][0].is_contiguous()
	hp = ADAM_B if kind == 'adam' else SGD_B
	hf, of, _ = _run(kind, True, [([0, 1], hp)], p0s, grads, sched=True)
	ht, ot, _ = _run(kind, False, [([0, 1], hp)], p0s, grads, sched=True)
	assert of.param_groups[0]['lr'] == ot.param_groups[0]['lr'] == hp['lr'] * 0.125
	h64 = _f64_run(kind, [hp, hp], p0s, grads, gamma=0.5)
	_report(f'{kind}, transposed gradient + StepLR, 3 steps', _hold_traj('transposed + StepLR', hf, ht, h64))


def test_sgd_state_dict_with_momentum_buffer_none():
	"""torch's own state dicts can hold momentum_buffer = None: it means no buffer yet, and the next step clones the gradient."""
	d = _draws(60, [(2100,)], 3)
	p0s, grads = [d[0][0]], [[d[0][1][k]] for k in range(3)]
	st = [dict(momentum_buffer=None)]
	hf, of, pf = _run('sgd', True, [([0], SGD_B)], p0s, grads, states=st)
	ht, _, _ = _run('sgd', False, [([0], SGD_B)], p0s, grads, states=st)
	assert of.state[pf[0]]['momentum_buffer'].shape == pf[0].shape
	h64 = _f64_run('sgd', [SGD_B], p0s, grads)
	_report('sgd, momentum_buffer = None loaded, 3 steps', _hold_traj('buffer None', hf, ht, h64))


@pytest.mark.parametrize('kind,kw', [('adam', dict(ADAM_B)), ('sgd', dict(SGD_A))])
def test_trajectory_of_200_steps_in_units(kind, kw):
	"""200 steps over three tensors (2049, 515 x 7, 1 element) with pre-drawn gradients that do not depend on the parameters, so the fused op, torch.optim
	and the float64 restatement walk the same path: error in units summed over the steps, worst over steps and entries."""
	shapes, steps = [(2049,), (515, 7), (1,)], 200
	rng = np.random.default_rng(70)
	p0s = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-3.0, 1.0, s)).astype(np.float32) for s in shapes]
	scale = [10.0 ** rng.uniform(-4.0, 1.0, s) for s in shapes]
	dev_g = [_t(((rng.standard_normal((steps,) + s) + 0.3) * sc).astype(np.float32)) for s, sc in zip(shapes, scale)]
	grads = [[gd[k] for gd in dev_g] for k in range(steps)]
	hp = {k: v for k, v in kw.items() if k != 'capturable'}
	hf, _, _ = _run(kind, True, [([0, 1, 2], kw)], p0s, grads)
	ht, _, _ = _run(kind, False, [([0, 1, 2], kw)], p0s, grads)
	host_g = [_n(gd) for gd in dev_g]
	h64 = _f64_run(kind, [hp] * 3, p0s, [[hg[k] for hg in host_g] for k in range(steps)])
	# one download per quantity and tensor, not one per step
	for h in (hf, ht):
		for i in range(3):
			for q in h[0][i]:
				stacked = torch.stack([row[i][q] for row in h]).cpu()
				for k, row in enumerate(h):
					row[i][q] = stacked[k]
	_report(f'{kind}{" capturable" if kw.get("capturable") else ""}, 200 steps', _hold_traj('200 steps', hf, ht, h64))


def test_c_abi_refusals_come_before_any_launch():
	"""Every refusal returns its error code and leaves the tensors as they were: nothing was launched.  Every pointer handed over is a live tensor
	of the stated size."""
	from find_amd import _lib
	L = _lib.lib()
	nt = 50
	ts = {k: [torch.full((4,), 0.5, device=DEV) for _ in range(nt)] for k in 'pgmv'}
	arr = {k: (ctypes.c_void_p * nt)(*[t.data_ptr() for t in v]) for k, v in ts.items()}
	numel = (ctypes.c_int64 * nt)(*([4] * nt))
	bad_numel = (ctypes.c_int64 * nt)(*([4] * (nt - 1) + [-1]))
	step_dev = torch.ones((), device=DEV)
	sd = ctypes.c_void_p(step_dev.data_ptr())
	s = _lib.current_stream(step_dev.device)

	def adam(n=1, step=1, b1=0.9, b2=0.999, eps=1e-8, m=arr['m'], v=arr['v'], ne=numel):
		return L.find_adam_step(n, arr['p'], arr['g'], m, v, ne, LR, b1, b2, eps, 0.0, step, s)

	def adam_dev(b1=0.9, b2=0.999, eps=1e-8, m=arr['m'], v=arr['v'], cnt=sd):
		return L.find_adam_step_dev(1, arr['p'], arr['g'], m, v, numel, LR, b1, b2, eps, 0.0, cnt, s)

	def sgd(mu=0.9, d=0.0, nes=0, bufs=arr['m']):
		return L.find_sgd_step(1, arr['p'], arr['g'], bufs, numel, LR, mu, d, 0.0, nes, 0, s)

	assert adam(step=0) == -1 and b'step counts from 1' in L.find_last_error()
	assert adam(step=-5) == -1
	assert adam(b1=1.0) == -1 and b'hyper-parameters' in L.find_last_error()
	assert adam(b2=1.0) == -1 and adam(b1=-0.1) == -1 and adam(b2=1.5) == -1
	assert adam(eps=-1e-8) == -1 and b'hyper-parameters' in L.find_last_error()
	assert adam(m=None) == -1 and b'NULL' in L.find_last_error()
	assert adam(v=None) == -1 and b'NULL' in L.find_last_error()
	assert adam(n=nt, ne=bad_numel) == -1 and b'bad tensor 49' in L.find_last_error()     # past the first launch of 48: still nothing launched
	assert adam_dev(cnt=None) == -1 and b'step_dev' in L.find_last_error()
	assert adam_dev(b1=1.0) == -1 and adam_dev(b2=1.0) == -1 and adam_dev(eps=-1.0) == -1 and b'hyper-parameters' in L.find_last_error()
	assert adam_dev(m=None) == -1 and adam_dev(v=None) == -1 and b'NULL' in L.find_last_error()
	assert sgd(bufs=None) == -1 and b'momentum needs its buffers' in L.find_last_error()
	assert sgd(nes=1, d=0.3) == -1 and b'Nesterov' in L.find_last_error()
	assert sgd(nes=1, mu=0.0) == -1 and b'Nesterov' in L.find_last_error()
	torch.cuda.synchronize()
	for k in ts:
		assert all(torch.equal(t, torch.full_like(t, 0.5)) for t in ts[k]), k
	assert adam(n=nt) == 0 and adam_dev() == 0 and sgd() == 0 and sgd(mu=0.0, bufs=None) == 0
	torch.cuda.synchronize()
	assert all(not torch.equal(t, torch.full_like(t, 0.5)) for t in ts['p']) and all(torch.equal(t, torch.full_like(t, 0.5)) for t in ts['g'])
