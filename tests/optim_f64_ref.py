"""Float64 restatement of the optimiser updates (torch/optim/adam.py::_single_tensor_adam, sgd.py::_single_tensor_sgd), an error unit
per entry, and the input generator that the host and the GPU tests of the fused optimisers share.  TEST INFRASTRUCTURE ONLY.

The restatement is plain numpy, float64 throughout, fed the fp32 inputs and the hyper-parameters as Python floats.  Beside the new state
each step returns a UNIT per entry and quantity: a first-order bound of what ONE fp32 evaluation of the same formula may be off by, built
from the float64 intermediates (E = 2^-24 is half an ulp, relative).  Tests assert error / unit, never an absolute or a relative error
of the parameter: a parameter of 0.7 that moves by 5e-4 hides a 4e-3 relative error of the update behind rtol = 2e-6.

Units (g' is the gradient after weight decay, u_g = E (|g| + |wd p|) its own rounding, 0 without weight decay):
  Adam   u_m = E (|m| + 2 |g'| + |wd p|)
         u_v = E v_new + 2 (1 - beta2) |g'| u_g                       (the second term: conditioning of g' = g + wd p)
         u_p = ulp32(p_new) / 2 + E |dp| + (step_size / denom) u_m + |dp| (sqrt(v_new / bc2) / denom) u_v / (2 v_new)
  SGD    u_buf = E (|mu buf| + |(1 - d) g'| + |wd p|)                 later steps;  u_g on the first step (the buffer is g' itself)
         u_p = ulp32(p_new) / 2 + E |dp| + lr (1 + mu [nesterov]) u_buf        (u_buf := u_g without momentum)

HOST_CAP bounds the error of a legitimate fp32 evaluation in these units.  It is counted, not measured: each rounding (of a result, or of
a hyper-parameter to fp32) is at most E relative to its own value, fused multiply-adds only remove roundings.
  m (cap 2):   d = g' - m, the weight w = 1 - beta1 rounded, w d, m + w d: at most E (|m| + 4 w (|g'| + |m|)), which is 1.8 units at
               w <= 0.2; torch's other lerp form (w >= 0.5: g' - d (1 - w)) gives at most E (3 |g'| + 2 |m|), 2 units; the rounding of g'
               is in the unit.
  v (cap 4):   beta2 rounded and v beta2 (2 E beta2 v), 1 - beta2 rounded, w g', (w g') g' (3 E w g'^2), the sum (E v_new): at most
               4 E v_new, plus the unit's conditioning term.
  p (cap 8):   v's error (at most 4 of its units) and m's (at most 2) enter through the unit's own last two terms; the update itself takes
               sqrt, bias_correction2_sqrt rounded, the division by it (torch: reciprocal and product), eps rounded and added, m / denom,
               step_size rounded, the product: 8 roundings of at most E |dp| each against the unit's one.
  buf (cap 4): mu rounded and mu buf, 1 - d rounded and (1 - d) g', the sum, and g' itself (2 E |wd p| + E |g'|): at most
               E (3 |mu buf| + 4 |(1 - d) g'| + 2 |wd p|); the first step's clone is g', at most 3 of its unit u_g.
  SGD p:       the buffer's 4 units through the last term, Nesterov's mu buf and sum one more each, lr rounded and the product 2 E |dp|:
               below the same cap 8.
A GPU test holds the fused op to 2 x torch.optim's own error in units; on the host path torch.optim's error is itself held to HOST_CAP
there, so GPU_CAP = 2 x HOST_CAP is the most a fused op can be off and pass."""
import numpy as np

E = 2.0 ** -24
HOST_CAP = dict(p=8.0, m=2.0, v=4.0, buf=4.0)
GPU_CAP = {k: 2.0 * c for k, c in HOST_CAP.items()}


def ulp32(x):
	"""Spacing of fp32 at |x| (float64 array in, float64 out; NaN stays NaN)."""
	with np.errstate(invalid='ignore', over='ignore'):
		return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _decayed(p, g, weight_decay):
	if weight_decay == 0:
		return g, np.zeros_like(g), np.zeros_like(g)
	wp = weight_decay * p
	return g + wp, np.abs(wp), E * (np.abs(g) + np.abs(wp))


def adam_step(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
	"""One dense Adam update in float64; `step` is the 1-based count including this update.
	Returns (p, m, v), (u_p, u_m, u_v).  With eps = 0 an entry with m_new = v_new = 0 is NaN, as in torch (0 / 0)."""
	p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
	b1, b2 = float(betas[0]), float(betas[1])
	gd, awp, u_g = _decayed(p, g, float(weight_decay))
	m_new = m + (gd - m) * (1.0 - b1)
	v_new = v * b2 + (1.0 - b2) * gd * gd
	step_size = lr / (1.0 - b1 ** step)
	s = np.sqrt(v_new) / (1.0 - b2 ** step) ** 0.5
	denom = s + eps
	with np.errstate(invalid='ignore', divide='ignore'):
		dp = step_size * (m_new / denom)
		p_new = p - dp
		u_m = E * (np.abs(m) + 2.0 * np.abs(gd) + awp)
		u_v = E * v_new + 2.0 * (1.0 - b2) * np.abs(gd) * u_g
		from_v = np.where(v_new > 0, np.abs(dp) * (s / denom) * u_v / (2.0 * np.where(v_new > 0, v_new, 1.0)), 0.0)
		u_p = 0.5 * ulp32(p_new) + E * np.abs(dp) + (step_size / denom) * u_m + from_v
	return (p_new, m_new, v_new), (u_p, u_m, u_v)


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
	"""One SGD update in float64; buf is None before the first step (torch clones the gradient, dampening ignored).
	Returns (p, buf), (u_p, u_buf); buf and u_buf are None without momentum."""
	p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
	gd, awp, u_g = _decayed(p, g, float(weight_decay))
	u_buf = u_g
	d = gd
	if momentum != 0:
		if buf is None:
			buf = gd.copy()
		else:
			buf = np.asarray(buf, dtype=np.float64)
			u_buf = E * (np.abs(momentum * buf) + np.abs((1.0 - dampening) * gd) + awp)
			buf = momentum * buf + (1.0 - dampening) * gd
		d = gd + momentum * buf if nesterov else buf
	dp = lr * d
	p_new = p - dp
	u_p = 0.5 * ulp32(p_new) + E * np.abs(dp) + lr * (1.0 + (momentum if nesterov else 0.0)) * u_buf
	return (p_new, buf if momentum != 0 else None), (u_p, u_buf if momentum != 0 else None)


def in_units(got, want, unit):
	"""|got - want| / unit per entry, float64.  An exact entry is 0 whatever its unit; an inexact one with unit 0 is inf; entries whose float64
	value is not finite are NaN (the caller compares their positions separately)."""
	got, want, unit = (np.asarray(a, dtype=np.float64) for a in (got, want, unit))
	with np.errstate(invalid='ignore', divide='ignore'):
		err = np.abs(got - want)
		r = np.where(err == 0, 0.0, err / unit)
	r = np.where(np.isfinite(want), np.where(np.isnan(r), np.inf, r), np.nan)
	return r


def worst(got, want, unit):
	"""max of in_units over the entries whose float64 value is finite (0 if there is none)."""
	r = in_units(got, want, unit)
	r = r[~np.isnan(r)]
	return float(r.max()) if r.size else 0.0


def make_inputs(n, seed=0):
	"""fp32 (p, g, m, v) of n elements for one update.
	|g| log-uniform in [1e-15, 1e4], random sign, every 97th entry exactly 0; p = randn * 10^U(-3, 1); previous moments in four interleaved
	kinds (entry i is of kind i % 4): 0 zero moments (a fresh state), 1 m = g (1 + 1e-3 randn) (cancels in the lerp), 2 m = -9 g (1 + 1e-4 randn)
	(the new m is about 0 at beta1 = 0.9), 3 m = g 10^U(-3, 3); v = g^2 10^U(-2, 2) for the kinds 1..3.  The floor of |g| keeps every non-zero
	v a normal fp32 number."""
	rng = np.random.default_rng(seed)
	g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15.0, 4.0, n)).astype(np.float32)
	g[::97] = 0.0
	p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 1.0, n)).astype(np.float32)
	g64 = g.astype(np.float64)
	kind = np.arange(n) % 4
	m = np.select([kind == 0, kind == 1, kind == 2], [np.zeros(n), g64 * (1.0 + 1e-3 * rng.standard_normal(n)), -9.0 * g64 * (1.0 + 1e-4 * rng.standard_normal(n))],
				  g64 * 10.0 ** rng.uniform(-3.0, 3.0, n)).astype(np.float32)
	v = np.where(kind == 0, 0.0, g64 * g64 * 10.0 ** rng.uniform(-2.0, 2.0, n)).astype(np.float32)
	assert np.all((v == 0) | (v >= np.finfo(np.float32).tiny))
	return p, g, m, v
