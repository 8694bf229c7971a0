"""The driver's contract for bench.py: one JSON line on stdout with the metric of BASELINE.json and the timing fields; a plain run
stops there, `--full` adds the roofline / cpu_baseline objects of the hot-path tier and the records of the other configurations."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields():
	r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--full', '--no-records'],
					   capture_output=True, text=True, timeout=900, cwd=ROOT)
	assert r.returncode == 0, r.stderr[-2000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
	assert len(lines) == 1, lines
	d = json.loads(lines[0])
	base = json.load(open(os.path.join(ROOT, 'BASELINE.json')))
	# BASELINE.json: "deformed vertices x rendered views / sec (fwd+bwd); Chamfer vs ref" -- the throughput clause is the bench metric
	assert d['metric'] == base['metric'].split(';')[0].replace('\u00d7', 'x').strip() and d['unit'] == 'vertices*views/s'
	assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1
	assert d['higher_is_better'] is True and d['scaling'] == 'weak' and d['data'] == 'synthetic' and d['dtype'].startswith('f32')
	assert d['vs_baseline'] is None   # BASELINE.md holds no published number for this metric
	assert d['value'] > 0 and d['ms_per_step'] > 0
	assert abs(d['value'] - 16 * 6890 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
	assert isinstance(d['config'].get('workload'), str) and 'model' not in d['config']
	rf = d['roofline']
	assert rf['bound'] in ('hbm', 'mfma') and rf['unit'] in ('GB/s', 'TFLOP/s')
	assert rf['peak'] > 0 and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9 and 0.3 < rf['frac'] < 1.0
	assert rf['traffic'] is None or rf['traffic'] > 0
	assert rf['avg_kernel_ms'] > 0 and rf['flops_per_launch'] > 0 and 'kernels' not in rf   # the per-kernel table lives in bench_records.json
	assert len(lines[0]) < 4096 and d['dtype'] == 'f32' and len(d['dtype_note']) < 200 and len(d['config']['workload']) <= 200
	full = json.load(open(os.path.join(ROOT, d['records_file'])))
	assert full['line']['value'] == d['value']
	ks = full['roofline_kernels']
	assert len(ks) >= 4 and all(k['isolated_us'] > 0 and 0.05 < k['frac'] < 1.0 for k in ks)
	cb = d['cpu_baseline']
	assert cb['value'] > 0 and cb['unit'] == d['unit'] and cb['cores'] >= 1 and cb['kind'] in ('reference', 'port') and isinstance(cb['sample'], str)


def test_a_plain_run_measures_the_headline_alone():
	"""Without --full the run sets up, primes, warms up, times the steps and prints the line: no roofline loop, CPU leg or records, no
	bench_records.json, and at most 30 s of the whole process's wall time outside its W + K steps."""
	import time
	rec = os.path.join(ROOT, 'bench_records.json')
	before = os.stat(rec).st_mtime_ns if os.path.exists(rec) else None
	steps, warmup = 20, 5
	t0 = time.perf_counter()
	r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
					   capture_output=True, text=True, timeout=600, cwd=ROOT)
	wall = time.perf_counter() - t0
	assert r.returncode == 0, r.stderr[-2000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
	assert len(lines) == 1, r.stdout[-2000:]
	d = json.loads(lines[0])
	assert d['n_gpus'] == 1 and d['steps'] == steps and d['warmup'] == warmup and d['dtype'] == 'f32' and d['higher_is_better'] is True
	assert d['unit'] == 'vertices*views/s' and abs(d['value'] - 16 * 6890 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
	assert not {'roofline', 'cpu_baseline', 'x_cpu_baseline', 'records', 'records_error', 'records_file', 'collective'} & set(d), sorted(d)
	assert not any(ln.startswith('{"record"') for ln in r.stderr.splitlines())
	assert (os.stat(rec).st_mtime_ns if os.path.exists(rec) else None) == before
	outside = wall - (steps + warmup) * d['ms_per_step'] * 1e-3
	assert outside <= 30.0, f'{outside:.1f} s outside the steps'


@pytest.mark.timeout(1200)
def test_the_drivers_exact_command_gives_one_short_parsable_line():
	"""round 4's line was 20.5 kB (15 nested records) and the driver could not parse it.  This runs the driver's command
	with --full -- records on, the longest line -- and holds it to what a parser with a small buffer can take: stdout is ONE line under 4 kB that carries the
	contract fields, the records travel as name -> [ms_per_step, steps] on the line, in full in bench_records.json and as one short JSON
	line each on stderr."""
	r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5', '--full'],
					   capture_output=True, text=True, timeout=1100, cwd=ROOT)
	assert r.returncode == 0, r.stderr[-2000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
	assert len(lines) == 1, r.stdout[-2000:]
	assert len(lines[0]) < 4096, len(lines[0])
	d = json.loads(lines[0])
	assert d['steps'] == 20 and d['warmup'] == 5 and d['n_gpus'] == 1 and d['dtype'] == 'f32'
	for k in ('metric', 'value', 'unit', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'data', 'config', 'roofline', 'cpu_baseline'):
		assert k in d, k
	for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'avg_kernel_ms', 'flops_per_launch', 'traffic'):
		assert k in d['roofline'], k
	for k in ('value', 'unit', 'cores', 'kind', 'sample'):
		assert k in d['cpu_baseline'], k
	assert len(d['config']['workload']) <= 200 and 'records_error' not in d
	names = {'train3d_b16_eager_colour_head', 'fp32_mfma', 'train3d_b1', 'train3d_b1_graph', 'c2', 'c3', 'c4_rank_share', 'c3_latlong_stress', 'c4_rank_share_latlong_stress', 'c5_fp32', 'c5_fp16'}
	assert names <= set(d['records']), sorted(d['records'])
	assert all(len(v) == 2 and v[0] > 0 and v[1] > 0 for v in d['records'].values())
	full = json.load(open(os.path.join(ROOT, d['records_file'])))
	assert set(full['records']) >= names and full['records']['c5_fp16']['roofline']['bound'] == 'hbm'
	# one short line per record on stderr
	rec_lines = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"record"')]
	assert {x['record'] for x in rec_lines} >= names
	assert all(len(ln) <= 1024 for ln in r.stderr.splitlines() if ln.startswith('{"record"'))


def test_two_rank_bench_path_runs_end_to_end_on_one_gpu():
	"""First execution of everything `bench.py --gpus N` does for N > 1 before the driver's own: spawn_ranks (fresh child
	processes with the launcher's environment; the parent never touches the GPU), init_from_env, the parameter broadcast, the gradient
	arena bucket + one all-reduce per step, the priming phase's cross-rank "go on" all-reduce, barrier-bracketed timing with the MAX over
	ranks, rank 0 alone printing the line.  FIND_BENCH_SHARE_GPU=1 puts both ranks on device 0 with gloo as the transport (this box has
	one GPU; RCCL itself runs in tests/test_gpu_distributed.py) -- the code path is the one the 8-GPU run takes."""
	env = dict(os.environ, FIND_BENCH_SHARE_GPU='1')
	for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
		env.pop(k, None)
	r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--full', '--no-records'],
					   capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
	assert r.returncode == 0, r.stderr[-3000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith('{')]
	assert len(lines) == 1, r.stdout[-2000:]
	d = json.loads(lines[0])
	assert d['n_gpus'] == 2 and d['steps'] == 3 and d['warmup'] == 1 and d['scaling'] == 'weak'
	assert d['config']['parallelism'] == 'dp2' and d['config']['feet_per_gpu'] == 16
	# whole-job aggregate: both ranks' feet over the slowest rank's time
	assert abs(d['value'] - 2 * 16 * 6890 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
	assert 'cpu_baseline' not in d and 'records' not in d   # rank 0 at N = 1 only
	assert d['roofline']['frac'] > 0.3
	# the line says what the exchange step saw: the process group's own world size, one entry per rank, the bucket, its time
	c = d['collective']
	assert c['backend'] == 'gloo' and c['world_size'] == 2 and len(c['ranks_devices']) == 2 and c['ranks_devices'][0].startswith('0:cuda:0')
	assert 3.4e6 < c['bucket_bytes'] < 4.0e6 and c['allreduce_us_per_step'] > 0
	# the MLP weights' part of the bucket (3.47 MB) went out inside the backward in every step of the run
	assert 3.4e6 < c['early_prefix_bytes'] < c['bucket_bytes'] and c['steps_with_early_prefix'] >= 3 + 1
	assert c['distinct_devices'] == 1   # (both ranks share device 0 in this test; the driver's run must show N)
	assert len(lines[0]) < 4096


def test_four_rank_bench_path_runs_end_to_end_on_one_gpu():
	"""`bench.py --gpus N` beyond two ranks: four ranks once, all on device 0 over gloo (FIND_BENCH_SHARE_GPU=1) -- the port choice,
	the store's time-outs with several children starting at different moments, the broadcast, one arena bucket per rank, the cross-rank
	"go on" of the priming phase, MAX-over-ranks timing, one line from rank 0 with a `collective` block that saw every rank (VERDICT r5
	item 8; the 1 -> 8 curve itself is the driver's to measure: processes time-slicing one GPU say nothing about throughput).  Four, not
	the driver's eight: a shared GPU host allows at most six processes with the device open, and this test process and bench.py's
	launcher may hold it beside the ranks."""
	n = 4
	env = dict(os.environ, FIND_BENCH_SHARE_GPU='1')
	for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
		env.pop(k, None)
	r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--steps', '2', '--warmup', '1', '--full', '--no-records', '--no-prime'],
					   capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
	assert r.returncode == 0, r.stderr[-3000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith('{')]
	assert len(lines) == 1, r.stdout[-2000:]
	d = json.loads(lines[0])
	assert d['n_gpus'] == n and d['steps'] == 2 and d['scaling'] == 'weak' and d['config']['parallelism'] == f'dp{n}'
	assert abs(d['value'] - n * 16 * 6890 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
	c = d['collective']
	assert c['world_size'] == n and len(c['ranks_devices']) == n and c['distinct_devices'] == 1
	assert [x.split(':')[0] for x in c['ranks_devices']] == [str(i) for i in range(n)]
	assert c['steps_with_early_prefix'] >= 2 + 1
	assert len(lines[0]) < 4096


def test_dump_outputs_hold_the_last_timed_step_and_do_not_depend_on_the_steps_before_it(tmp_path):
	"""--dump-outputs: the loss and its terms, every trainable parameter after the last timed step's optimiser step and the gradient it holds,
	as float32 .npy files, 64 MB at most in all.  That step starts from the state setup left, so two runs with the same arguments, and a
	single unprimed step, agree up to the rounding of one step: float atomics in the backward of the surface sampling and the Chamfer term
	(tests/test_gpu_trainloop.py), which Adam's first step turns into lr * sign(gradient) on entries whose gradient is rounding noise.  Without
	the restore, the 125 steps of the default command left losses 6e-4 apart and gradients 30 % of their tensor's largest entry."""
	import numpy as np
	lr = 5e-5   # the headline's Adam lr (bench.train3d_setup)

	def dump(name, *args):
		d = tmp_path / name
		r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--headline-only', '--dump-outputs', str(d), *args],
						   capture_output=True, text=True, timeout=600, cwd=ROOT)
		assert r.returncode == 0, r.stderr[-3000:]
		return {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}

	def differences(x, y):
		"""What does not agree within the rounding of one step (empty: the two dumps agree)."""
		assert set(x) == set(y)
		bad = [k for k in x if k.startswith('loss') and abs(float(x[k]) - float(y[k])) > 1e-5 * abs(float(x[k]))]
		bad += [k for k in x if k.startswith('grad.') and np.abs(x[k] - y[k]).max() > 1e-2 * np.abs(x[k]).max()]
		d = np.concatenate([np.abs(x[k] - y[k]).ravel() for k in x if k.startswith('param.')])
		if (d > 0.1 * lr).mean() > 1e-3 or d.max() > 2 * lr:   # (a flipped sign: lr one way against lr the other)
			bad.append(f'params: {(d > 0.1 * lr).mean():.2e} of the entries more than 0.1 lr apart, the furthest {d.max():.2e}')
		return bad

	a = dump('a', '--steps', '20', '--warmup', '5', '--repeats', '2')
	b = dump('b', '--steps', '20', '--warmup', '5', '--repeats', '2')
	single = dump('single', '--steps', '1', '--warmup', '0', '--repeats', '1', '--no-prime')
	assert {'loss', 'loss_chamf', 'loss_smooth', 'loss_tex', 'param.model.base.0.weight', 'grad.model.base.0.weight', 'grad.model.reg.data'} <= set(a)
	assert all(k.startswith(('loss', 'param.', 'grad.')) for k in a)
	assert all('param.' + k[5:] in a and a[k].shape == a['param.' + k[5:]].shape for k in a if k.startswith('grad.'))
	assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
	assert sum(v.nbytes for v in a.values()) <= 64 << 20
	assert abs(float(a['loss']) - sum(float(a[k]) for k in ('loss_chamf', 'loss_smooth', 'loss_tex'))) <= 1e-5 * abs(float(a['loss']))
	assert differences(a, b) == []
	assert differences(a, single) == []
