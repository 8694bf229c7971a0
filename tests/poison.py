"""Poisoned allocations for the HIP path's Python wrappers.

Every workspace, output and gradient buffer of find_amd.functional, functional_render, vis and optim is torch.empty / torch.empty_like:
memory the caching allocator hands back as the previous call left it.  A test that runs one shape twice therefore gives a kernel that
forgets to write a region the correct stale values of the call before.  `poisoned(byte)` makes such a region visible: while it is
active, every torch.empty / torch.empty_like issued from those four modules (so also _ws, _grad_for and _fill_rest) comes back with all
of its bytes set to `byte`.

Two patterns, which complement each other, and no other:
  0xFF  NaN as a float, -1 as an int32, ~0 as a 64-bit key.  NaN survives a multiplication by a zero weight.
  0x00  0.0, index 0, key 0.  ~0 and -1 are the kernels' own "nothing found" values, so 0xFF hides a forgotten key preset; a key of 0
        wins every minimum and exposes one.
Neither decodes to a large integer: an index misread from poison is -1 or 0.  The aim is wrong numbers, not out-of-bounds accesses.

The mechanism is a proxy for the module-level name `torch` of each module, not a TorchDispatchMode: a dispatch mode is thread-local,
and autograd runs the backward of GPU tensors on its device thread.

`compare(name, r0, r1, r2, rules)` is the comparison the GPU cases (tests/test_gpu_poison.py) and the harness's own self-test share."""
import contextlib
import importlib

import torch

MODULES = ('find_amd.functional', 'find_amd.functional_render', 'find_amd.vis', 'find_amd.optim')
PATTERNS = (0xFF, 0x00)


def _fill(t, byte):
	if t.numel():
		# (a contiguous fresh allocation: its bytes as one flat uint8 view; preserve_format may give a dense permuted layout, whose
		# storage is still exactly numel elements)
		flat = t.as_strided((t.numel(),), (1,), t.storage_offset())
		flat.view(torch.uint8).fill_(byte)
	return t


class _TorchProxy:
	"""Stands in for the module `torch`: every attribute is the real one, except empty / empty_like, which fill what they allocate."""

	def __init__(self, byte):
		self.__dict__['_byte'] = byte
		self.__dict__['calls'] = 0

	def __getattr__(self, name):
		return getattr(torch, name)

	def __setattr__(self, name, value):
		setattr(torch, name, value)

	def empty(self, *args, **kwargs):
		self.__dict__['calls'] += 1
		return _fill(torch.empty(*args, **kwargs), self._byte)

	def empty_like(self, *args, **kwargs):
		self.__dict__['calls'] += 1
		return _fill(torch.empty_like(*args, **kwargs), self._byte)


@contextlib.contextmanager
def poisoned(byte):
	"""Every torch.empty / torch.empty_like of the HIP path's wrapper modules returns memory filled with `byte` (0xFF or 0x00)."""
	if byte not in PATTERNS:
		raise ValueError(f'poisoned: the patterns are 0xFF and 0x00, got {byte!r}')
	mods = [importlib.import_module(m) for m in MODULES]
	for m in mods:
		if m.torch is not torch:
			raise RuntimeError(f'poisoned: {m.__name__}.torch is already replaced (nested use)')
	proxy = _TorchProxy(byte)
	try:
		for m in mods:
			m.torch = proxy
		yield proxy
	finally:
		for m in mods:
			m.torch = torch


# ------------------------------------------------------------------------------------------------ comparison
class Rule:
	"""How one quantity of a case's result is compared between the clean and the poisoned runs.
	bits    True: torch.equal.  False: a float-atomic sum; then one of
	rel     |a - b| <= rel * max(largest |clean| entry, floor), or
	abs     |a - b| <= abs: a bound the suite already holds two correct runs of the op to (the scale of `rel` only sizes the bound the
	        way that test sizes it: the figure itself is the suite's), or
	bound   a tensor (broadcastable to the quantity) of absolute bounds derived from a float64 restatement of the addends.
	irange  for integer quantities: (lo, hi) -- every value is -1 or in [lo, hi)."""

	def __init__(self, bits=True, rel=None, abs=None, bound=None, irange=None, floor=1e-30):
		self.bits, self.rel, self.abs, self.bound, self.irange, self.floor = bits, rel, abs, bound, irange, floor
		if not bits and rel is None and abs is None and bound is None:
			raise ValueError('Rule: a quantity that is not bit-equal needs rel, abs or bound')


BITS = Rule()


def atomic_bound(n_row, sum_abs):
	"""(n_row + 3) * 2^-24 * sum|addend| per row: n_row float additions in any order (each result within 2^-24 of its exact value,
	partial sums bounded by sum|addend|) plus three roundings in forming an addend."""
	return (n_row.double() + 3.0) * 2.0 ** -24 * sum_abs.double()


def compare(name, r0, r1, r2, rules=None):
	"""r0: the clean run's dict of tensors; r1, r2: the runs under poisoned(0xFF) / poisoned(0x00).  Returns the list of violations
	(strings; empty = the case holds): a quantity missing from a run, poison that survives (a non-finite float where the clean run is
	finite, an integer outside its op's range), or a difference beyond the quantity's rule."""
	rules = rules or {}
	bad = []
	for key, a in r0.items():
		rule = rules.get(key, BITS)
		for tag, r in (('0xFF', r1), ('0x00', r2)):
			b = r.get(key)
			if (a is None) != (b is None):
				bad.append(f'{name}/{key} [{tag}]: {"missing" if b is None else "unexpected"}')
				continue
			if a is None:
				continue
			if a.shape != b.shape or a.dtype != b.dtype:
				bad.append(f'{name}/{key} [{tag}]: {tuple(b.shape)} {b.dtype} instead of {tuple(a.shape)} {a.dtype}')
				continue
			if a.numel() == 0:
				continue
			if a.is_floating_point():
				lost = torch.isfinite(a) & ~torch.isfinite(b)
				if lost.any():
					bad.append(f'{name}/{key} [{tag}]: {int(lost.sum())} of {a.numel()} entries are not finite (first at flat index {int(lost.flatten().nonzero()[0])})')
					continue
			elif rule.irange is not None:
				lo, hi = rule.irange
				for t, who in ((a, 'clean'), (b, tag)):
					out = (t != -1) & ((t < lo) | (t >= hi))
					if out.any():
						bad.append(f'{name}/{key} [{who}]: {int(out.sum())} integer entries outside -1 / [{lo}, {hi})')
			if rule.bits:
				if not torch.equal(a, b) and not (a.is_floating_point() and _equal_with_nan(a, b)):
					diff = a != b
					bad.append(f'{name}/{key} [{tag}]: {int(diff.sum())} of {a.numel()} entries differ from the clean run (first at flat index {int(diff.flatten().nonzero()[0])})')
			else:
				err = (a.double() - b.double()).abs()
				if rule.bound is not None:
					lim = rule.bound.to(err.device).double().expand_as(err)
				elif rule.abs is not None:
					lim = torch.full_like(err, rule.abs)
				else:
					lim = torch.full_like(err, rule.rel * max(float(a.abs().max()), rule.floor))
				over = err > lim
				if over.any():
					bad.append(f'{name}/{key} [{tag}]: {int(over.sum())} entries beyond the summation-order bound, worst {float((err - lim).max()):.3e} over it (max |diff| {float(err.max()):.3e})')
	return bad


def _equal_with_nan(a, b):
	"""Bit-for-bit agreement where the clean run itself is not finite (it must then be non-finite in the same places)."""
	fa, fb = torch.isfinite(a), torch.isfinite(b)
	return bool(torch.equal(fa, fb)) and bool(torch.equal(a[fa], b[fb])) and bool(torch.equal(torch.isnan(a), torch.isnan(b)))
