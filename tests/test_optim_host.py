"""The yardstick of the fused optimisers' GPU tests, checked on the CPU: tests/optim_f64_ref.py (float64 restatement + error unit + input
generator) reproduces torch.optim's own trajectories, a correct fp32 evaluation (oracle/optim_ref.py) stays within HOST_CAP units on the
generator's inputs, and every subtly wrong update below lands at least ten times beyond what a GPU test lets pass."""
import itertools

import numpy as np
import pytest

from oracle import optim_ref
from tests import optim_f64_ref as R
from tests.test_oracle_optim import CASES, GOLD, SHAPES, STEPS

F = np.float32
N = 200_000
LR = 3e-3                     # distinct from every other hyper-parameter
ADAM_CASES = list(itertools.product((1, 2, 10, 1000), (1e-8, 1e-3, 0.0), (0.0, 0.01)))    # step, eps, weight_decay
SGD_CASES = [(mu, d, wd, nes) for mu, d, wd, nes in itertools.product((0.0, 0.9), (0.0, 0.3), (0.0, 0.05), (False, True))
			 if not (nes and (mu == 0 or d != 0)) and not (mu == 0 and d != 0)]


@pytest.fixture(scope='module')
def inputs():
	return R.make_inputs(N, seed=0)


@pytest.fixture(scope='module')
def gold():
	return np.load(GOLD)


def _adam32(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, mutant=None):
	"""oracle/optim_ref.adam_step with one deliberate mistake switched on by `mutant` (None: the oracle itself, bit for bit)."""
	p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
	b1, b2 = betas
	g_raw = g
	if weight_decay != 0:
		if mutant == 'adamw':
			p = p * F(1.0 - lr * weight_decay)
		else:
			g = g + F(weight_decay) * p
	m = m + (g - m) * F(1.0 - b1)
	gv = g_raw if mutant == 'v_before_wd' else g
	v = v * F(b2) + (F(1.0) - F(b2) if mutant == 'one_minus_beta2_in_fp32' else F(1.0 - b2)) * gv * gv
	bc1 = 1.0 - b1 ** (step - 1 if mutant == 'bc1_prev_step' else step)
	bc2 = 1.0 if mutant == 'no_bc2' else 1.0 - b2 ** step
	step_size = F(lr / bc1)
	if mutant == 'eps_in_sqrt':
		denom = np.sqrt(v + F(eps)) / F(bc2 ** 0.5)
	else:
		denom = np.sqrt(v) / F(bc2 ** 0.5) + F(eps * 1.01 if mutant == 'eps_1.01' else eps)
	p = p - step_size * (m / denom)
	return p.astype(F), m.astype(F), v.astype(F)


def _sgd32(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, mutant=None):
	p, g = np.asarray(p, dtype=F), np.asarray(g, dtype=F)
	if weight_decay != 0 and mutant != 'wd_after_momentum':
		g = g + F(weight_decay) * p
	if momentum != 0:
		if buf is None:
			buf = g * F(1.0 - dampening) if mutant == 'dampen_first' else g.copy()
		else:
			buf = np.asarray(buf, dtype=F) * F(momentum) + F(1.0 - dampening) * g
		g = buf if (mutant == 'nesterov_buf_alone' or not nesterov) else g + F(momentum) * buf
	if weight_decay != 0 and mutant == 'wd_after_momentum':
		g = g + F(weight_decay) * p
	p = p - F(lr) * g
	return p.astype(F), (None if buf is None else buf.astype(F))


def _adam_units(inputs, fn, step, eps, wd, **kw):
	p, g, m, v = inputs
	with np.errstate(invalid='ignore', divide='ignore'):
		(P, M, V), (up, um, uv) = R.adam_step(p, g, m, v, step, lr=LR, eps=eps, weight_decay=wd)
		p1, m1, v1 = fn(p, g, m, v, step, lr=LR, eps=eps, weight_decay=wd, **kw)
	assert np.array_equal(np.isfinite(p1), np.isfinite(P))
	return dict(p=R.worst(p1, P, up), m=R.worst(m1, M, um), v=R.worst(v1, V, uv)), P


def _sgd_units(inputs, fn, first, mu, d, wd, nes, **kw):
	p, g, m, _ = inputs
	buf = None if (first or mu == 0) else m
	(P, B), (up, ub) = R.sgd_step(p, g, buf, LR, mu, d, wd, nes)
	p1, b1 = fn(p, g, buf, LR, mu, d, wd, nes, **kw)
	assert (B is None) == (b1 is None) == (mu == 0)
	return dict(p=R.worst(p1, P, up), buf=0.0 if B is None else R.worst(b1, B, ub))


@pytest.mark.parametrize('name', sorted(CASES))
def test_f64_restatement_reproduces_torch_trajectories(gold, name):
	"""torch.optim's own fp32 trajectories (tests/golden/optim.npz) stay within HOST_CAP x the units summed over the steps taken."""
	kind, kw = CASES[name]
	for i in range(SHAPES):
		p = gold[f'p0/{i}'].astype(np.float64)
		m = np.zeros_like(p); v = np.zeros_like(p); buf = None
		acc = np.zeros_like(p)
		for k in range(STEPS):
			g = gold[f'grad/{k}/{i}']
			if kind == 'adam':
				(p, m, v), (up, _, _) = R.adam_step(p, g, m, v, k + 1, **kw)
			else:
				(p, buf), (up, _) = R.sgd_step(p, g, buf, **kw)
			acc += up
			w = R.worst(gold[f'{name}/{k}/{i}'], p, acc)
			assert w <= R.HOST_CAP['p'], (name, i, k, w)


def test_restated_oracle_is_the_oracle(inputs):
	p, g, m, v = inputs
	for a, b in zip(_adam32(p, g, m, v, 10, LR, eps=1e-3, weight_decay=0.01), optim_ref.adam_step(p, g, m, v, 10, lr=LR, eps=1e-3, weight_decay=0.01)):
		assert np.array_equal(a, b)
	for buf in (None, m):
		for a, b in zip(_sgd32(p, g, buf, LR, 0.9, 0.3, 0.05), optim_ref.sgd_step(p, g, buf, LR, 0.9, 0.3, 0.05)):
			assert np.array_equal(a, b)


def test_generator_ranges(inputs):
	p, g, m, v = inputs
	nz = g != 0
	assert np.all(g[::97] == 0) and np.abs(g[nz]).min() >= 1e-15 and np.abs(g[nz]).max() <= 1e4 and np.abs(g[nz]).min() < 1e-14 and np.abs(g[nz]).max() > 1e3
	assert all(a.dtype == F for a in inputs)
	kind = np.arange(N) % 4
	assert np.all(m[kind == 0] == 0) and np.all(v[kind == 0] == 0)
	assert np.all(np.abs(m[(kind == 1) & nz] / g[(kind == 1) & nz] - 1) < 1e-2)
	assert np.all(np.abs(m[(kind == 2) & nz] / g[(kind == 2) & nz] + 9) < 1e-2)
	assert np.all(v[(kind != 0) & nz] >= np.finfo(F).tiny)


@pytest.mark.parametrize('step,eps,wd', ADAM_CASES)
def test_fp32_adam_is_within_cap_on_the_generated_inputs(inputs, step, eps, wd):
	"""Condition on the inputs: a correct fp32 evaluation is within HOST_CAP units of the float64 restatement for p, m and v; with eps = 0 the
	non-finite entries are exactly those with g = m = v = 0 (0 / 0), none once weight decay makes the gradient non-zero."""
	w, P = _adam_units(inputs, _adam32, step, eps, wd)
	print(f'adam step={step} eps={eps} wd={wd}: ' + ' '.join(f'{k} {x:.2f}' for k, x in w.items()))
	for k, x in w.items():
		assert x <= R.HOST_CAP[k], (k, x)
	p, g, m, v = inputs
	dead = (g == 0) & (m == 0) & (v == 0) & ((p == 0) | (wd == 0))
	assert np.array_equal(~np.isfinite(P), dead if eps == 0 else np.zeros(N, bool))
	if eps == 0 and wd == 0:
		assert dead.sum() == len(range(0, N, 97))


@pytest.mark.parametrize('mu,d,wd,nes', SGD_CASES)
@pytest.mark.parametrize('first', (True, False))
def test_fp32_sgd_is_within_cap_on_the_generated_inputs(inputs, first, mu, d, wd, nes):
	w = _sgd_units(inputs, _sgd32, first, mu, d, wd, nes)
	print(f'sgd first={first} mu={mu} d={d} wd={wd} nesterov={nes}: ' + ' '.join(f'{k} {x:.2f}' for k, x in w.items()))
	for k, x in w.items():
		assert x <= R.HOST_CAP[k], (k, x)


@pytest.mark.parametrize('mutant', ['eps_1.01', 'eps_in_sqrt', 'no_bc2', 'bc1_prev_step', 'adamw', 'v_before_wd', 'one_minus_beta2_in_fp32'])
def test_adam_mutant_is_caught(inputs, mutant):
	"""Each mistake, applied to the fp32 oracle, exceeds 10 x GPU_CAP (the most a GPU test lets pass) in at least one case and quantity."""
	best = 0.0
	for step, eps, wd in ADAM_CASES:
		if eps == 0 or (mutant == 'bc1_prev_step' and step == 1):   # (step - 1 = 0: the mutant divides by 0, caught trivially)
			continue
		w, _ = _adam_units(inputs, _adam32, step, eps, wd, mutant=mutant)
		best = max(best, max(w[k] / R.GPU_CAP[k] for k in w))
	print(f'{mutant}: {best:.3g} x GPU_CAP')
	assert best >= 10.0, (mutant, best)


@pytest.mark.parametrize('mutant', ['dampen_first', 'nesterov_buf_alone', 'wd_after_momentum'])
def test_sgd_mutant_is_caught(inputs, mutant):
	best = 0.0
	for first in (True, False):
		for mu, d, wd, nes in SGD_CASES:
			w = _sgd_units(inputs, _sgd32, first, mu, d, wd, nes, mutant=mutant)
			best = max(best, max(w[k] / R.GPU_CAP[k] for k in w))
	print(f'{mutant}: {best:.3g} x GPU_CAP')
	assert best >= 10.0, (mutant, best)
