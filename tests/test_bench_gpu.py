"""bench.py end to end: the single-GPU line the driver records, and the N = 2 launch exactly as the driver starts it
(`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`) with both ranks on the box's one GPU and
gloo as transport (RCCL refuses two ranks on one device) -- reducers, comm stream, barrier + max-over-ranks timing."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _json_line(out, full=None):
    """The compact stdout line (the driver parses the LAST line; it keeps ~16 KB of stdout), merged over the full record
    of the side file when `full` names it: the line's own fields win, so every check below also checks the line."""
    lines = [l for l in out.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and out.rstrip().splitlines()[-1] == lines[0], out[-2000:]
    assert len(lines[0]) < 8000, len(lines[0])
    line = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'full_record'):
        assert k in line, k
    if full is None:
        return line
    rec = json.load(open(full))
    for k, v in line.items():          # the line is a rounded excerpt of the record
        if k in ('sub', 'full_record', 'kernel_ms_per_step'):
            continue
        if isinstance(v, float):
            assert abs(v - rec[k]) <= 1e-3 * abs(rec[k]) + 1e-4, k
        elif isinstance(v, dict):
            for kk, vv in v.items():
                if isinstance(vv, float):
                    assert abs(vv - rec[k][kk]) <= 1e-3 * abs(rec[k][kk]) + 1e-4, (k, kk)
    for name, sr in line.get('sub', {}).items():
        assert abs(sr['ms_per_step'] - rec['sub'][name]['ms_per_step']) < 1e-3
    rec['_line'] = line
    return rec


def _check(d, world, steps=2, warmup=1):
    assert d['n_gpus'] == world and d['steps'] == steps and d['warmup'] == warmup
    assert d['unit'] == 'steps/s' and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['value'] > 0 and abs(d['value'] - world * 1000.0 / d['ms_per_step']) < 1e-4 * d['value']
    # the blocks are timed by events inside ONE synchronised window of `steps` steps: the window's wall clock per step agrees
    assert 0.5 * d['ms_per_step'] < d['wall_ms_per_step'] < 2.0 * d['ms_per_step'] and sum(d['blocks_steps']) == steps
    assert d['final_loss'] == d['final_loss'] and abs(d['final_loss']) < 1e9
    assert d['config']['global_batch'] == 64 * world and d['dtype'].startswith('f32')
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and r['unit'] == 'TFLOP/s' and r['achieved'] > 0
    # default products = 6 bf16 MFMA products per fp32 product: priced against the fp32 MFMA peak AND the bf16 peak / 6
    assert 'bf16x6' in d['dtype'] and r['peak'] == 157.3 and abs(r['peak_bf16_div6'] - 2500.0 / 6) < 1e-6
    assert abs(r['frac_bf16_div6'] - r['achieved'] / r['peak_bf16_div6']) < 1e-9 and r['executed']['mfma_tflops'] > r['achieved']


@pytest.mark.parametrize('workload', ['train_vqa', 'search_vqa', 'arch_vqa'])
def test_bench_single_gpu(workload, tmp_path):
    full = str(tmp_path / 'full.json')
    p = subprocess.run([sys.executable, 'bench.py', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--workload', workload,
                        '--full-out', full], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _json_line(p.stdout, full)
    _check(d, 1)
    assert ('supernet' in d['metric']) == (workload != 'train_vqa')   # the label follows the workload


def test_bench_default_line_is_the_supernet_weight_step_with_sub_records():
    """The --full command without --workload: headline = the BASELINE metric's workload, the other three under `sub`,
    every record with its own roofline and CPU baseline -- in the side file; the LINE stays under 8000 characters with
    `roofline`, `cpu_baseline` and one short object per sub record, and stderr stays quiet."""
    env = dict(os.environ, NCCL_DEBUG='VERSION')   # (RCCL would print a version banner to stdout from the one-rank records)
    env.pop('HIP_FORCE_DEV_KERNARG', None)         # bench.py sets it itself and records it
    full = os.path.join(ROOT, 'bench_full.json')
    if os.path.exists(full):
        os.remove(full)
    p = subprocess.run([sys.executable, 'bench.py', '--full', '--steps', '30', '--warmup', '1', '--cpu-budget', '3'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(p.stderr.splitlines()) < 20, p.stderr[-3000:]
    d = _json_line(p.stdout, full)
    line = d['_line']
    assert line['full_record'] == 'bench_full.json' and line['config']['hip_force_dev_kernarg'] == '1'
    assert 'NCCL_DEBUG' not in line['config']['rccl_env']
    assert line['cpu_baseline']['kind'] == 'port' and line['cpu_baseline']['value'] > 0 and 0 < line['roofline']['frac'] < 1
    # round 6: what LIMITS the d = 256 GEMM class is in the line -- the measured share of per-launch fixed
    # cost -- and the fraction of the pipe the products execute on stands next to `frac`; the library, not bench.py, set the
    # kernel-argument placement
    rl = line['roofline']
    assert rl['bound'] == 'mfma' and rl['limited_by'] in ('latency / fixed cost', 'mfma issue (K loop)')
    assert 0.01 < rl['fixed_cost_share'] < 0.95 and 0.5 < rl['fixed_cost_us_per_launch'] < 20.0 and 0 < rl['frac_bf16_div6'] < rl['frac']
    assert line['config']['hip_force_dev_kernarg_source'] == 'set_by_library'
    assert set(line['sub']) == set(d['sub']) and all(s['value'] > 0 and s['ms_per_step'] > 0 for s in line['sub'].values())
    assert [l for l in p.stdout.splitlines() if l.strip()] == [l for l in p.stdout.splitlines() if l.startswith('{')], \
        'stdout must carry the one JSON line and nothing else: ' + p.stdout[-500:]
    _check(d, 1, steps=30)
    assert d['metric'].startswith('supernet fwd+bwd steps/sec') and 'WEIGHT step' in d['config']['workload']
    main = {'arch_step', 'bilevel', 'train_vqa'}
    n1 = {'search_vqa_stream', 'search_vqa_dropin', 'search_vqa_dp1', 'train_vqa_dp1'}     # N = 1 only: short records
    unpad = {'search_vqa_unpad', 'train_vqa_unpad'}                                         # N = 1 only: the ragged decoder stream
    assert set(d['sub']) == main | n1 | unpad
    for k in unpad:
        r = d['sub'][k]
        assert r.get('error') is None and r['value'] > 0 and 0 < r['roofline']['frac'] < 1 and 0.5 < r['ms_per_step_vs_plain'] < 1.02, (k, r.get('ms_per_step_vs_plain'))
    for r in [d] + [d['sub'][k] for k in main]:
        assert r['value'] > 0 and 0 < r['roofline']['frac'] < 1
        assert r['repeats'] == 5 and r['value_min'] <= r['value'] <= r['value_max']   # median of five timed blocks
        assert sum(r['blocks_steps']) == r['steps'] and len(r['blocks_ms_per_step']) == 5   # that together make --steps
        cb = r['cpu_baseline']
        assert cb['kind'] == 'port' and cb['value'] > 0 and cb['cores'] >= 1 and cb['unit'] == 'steps/s'
    assert d['sub']['bilevel']['steps'] == 30
    for k in n1:
        r = d['sub'][k]
        assert r.get('error') is None and r['value'] > 0 and r['host_issue_ms_per_step'] > 0 and r['library_launches_per_step'] > 100, (k, r)
    # the exchange machinery really ran: RCCL, one rank, collectives forced
    for k in ('search_vqa_dp1', 'train_vqa_dp1'):
        assert d['sub'][k]['config'] == {'grad_allreduce': 'rccl', 'rccl_ranks': 1, 'force_collectives': True}
        assert 0.8 < d['sub'][k]['ms_per_step_vs_plain'] < 1.5    # (1.02-1.07 measured; the plain record is the first 0.15 s of GPU work of a cold process: +-10 %)
    assert d['sub']['search_vqa_stream']['ms_per_step_vs_plain'] < 1.25
    tp = d['roofline']['traffic_pmc']
    assert tp is None or 'source_commit' in tp


def _same_outputs(a, b):
    """Two --dump-outputs of the same steps: the same sampled operators, loss and gradients up to run-to-run round-off."""
    import numpy as np
    return (np.array_equal(a['sampled_ops'], b['sampled_ops']) and abs(a['loss'][0] - b['loss'][0]) <= 1e-5 * abs(a['loss'][0])
            and np.allclose(a['grad_norms'], b['grad_norms'], rtol=1e-4, atol=1e-6 * a['grad_norms'].max())
            and np.abs(a['grad_sample'] - b['grad_sample']).max() <= 1e-4 * np.abs(a['grad_sample']).max())


def _load_outputs(out):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """The plain command (no --full) does only what the headline needs: one JSON line with the contract's fields for the
    supernet weight step alone -- no sub records, empty-queue host time, roofline pass or CPU baseline, and no side file --
    and its timed steps compute what the same steps of a --full run compute."""
    side = os.path.join(ROOT, 'bench_full.json')
    if os.path.exists(side):
        os.remove(side)
    plain = str(tmp_path / 'plain')
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', plain],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['repeats'] == 3
    assert d['unit'] == 'steps/s' and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['value'] > 0 and abs(d['value'] - 1000.0 / d['ms_per_step']) < 1e-4 * d['value']
    assert d['value_min'] <= d['value'] <= d['value_max'] and d['final_loss'] == d['final_loss']
    assert d['metric'].startswith('supernet fwd+bwd steps/sec') and 'WEIGHT step' in d['config']['workload']
    assert 'bf16x6' in d['dtype'] and d['config']['global_batch'] == 64 and d['full_record'] is None
    for k in ('sub', 'roofline', 'hbm_kernels', 'kernel_ms_per_step', 'cpu_baseline', 'gpu_vs_cpu', 'host_issue_ms_per_step_empty_queue'):
        assert k not in d, k
    assert not os.path.exists(side)
    got = _load_outputs(plain)
    assert sorted(got) == ['grad_norms', 'grad_sample', 'loss', 'sampled_ops']
    assert abs(got['loss'][0] - d['final_loss']) <= 1e-6 * abs(d['final_loss'])
    full = str(tmp_path / 'full')
    p = subprocess.run([sys.executable, 'bench.py', '--full', '--workload', 'search_vqa', '--steps', '3', '--warmup', '1',
                        '--no-cpu-baseline', '--no-fixed-cost', '--full-out', full + '.json', '--dump-outputs', full],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _same_outputs(got, _load_outputs(full))


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """--dump-outputs: float32 / float64 arrays under 64 MB -- the loss the line reports, per-parameter gradient norms, the
    seeded gradient sample, the sampled operators.  The same arguments give the same outputs; so does the same number of
    steps split differently between warm-up and timed steps (--steps is exactly the timed steps, and nothing runs between the
    last of them and the dump); one step more gives other outputs."""
    import numpy as np

    def run(steps, warmup, out):
        p = subprocess.run([sys.executable, 'bench.py', '--workload', 'search_vqa', '--steps', str(steps), '--warmup', str(warmup),
                            '--no-cpu-baseline', '--no-fixed-cost', '--full-out', str(out) + '.json',
                            '--dump-outputs', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        d = _json_line(p.stdout, str(out) + '.json')
        assert d['steps'] == steps and sum(d['blocks_steps']) == steps
        files = sorted(os.listdir(str(out)))
        assert files == ['grad_norms.npy', 'grad_sample.npy', 'loss.npy', 'sampled_ops.npy'], files
        got = {f[:-4]: np.load(os.path.join(str(out), f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(os.path.getsize(os.path.join(str(out), f)) for f in files) <= 64 << 20
        assert d['outputs'] == {k: list(a.shape) for k, a in got.items()}
        assert got['loss'][0] == d['final_loss'] and got['sampled_ops'].shape == (30,)
        assert got['grad_sample'].size > 1 << 21 and np.isfinite(got['grad_sample']).all() and (got['grad_norms'] > 0).any()
        return got

    base = tmp_path / 'out'
    a, b = run(3, 1, str(base) + 'a'), run(3, 1, str(base) + 'b')
    assert _same_outputs(a, b)
    assert _same_outputs(a, run(2, 2, str(base) + 'c'))             # step 4 of the run either way
    assert not _same_outputs(a, run(4, 1, str(base) + 'd'))         # step 5


def test_bench_gpus_flag_must_match_the_launch():
    """--gpus N under a launcher that started a different number of ranks is refused, never mislabelled."""
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '2', '--steps', '1', '--warmup', '0', '--no-cpu-baseline',
                        '--workload', 'search_vqa'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and 'WORLD_SIZE' in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith('{')]


def test_bench_gpus_flag_self_spawns_ranks(tmp_path):
    """--gpus 2 without a launcher starts the two ranks itself (here both on the one GPU, gloo transport)."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(MMNAS_BENCH_BACKEND='gloo', MMNAS_BENCH_DEVICE='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '2', '--steps', '2', '--warmup', '1', '--no-cpu-baseline',
                        '--workload', 'search_vqa', '--full-out', str(tmp_path / 'f.json')], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    d = _json_line(p.stdout, str(tmp_path / 'f.json'))
    _check(d, 2)
    assert d['config']['rccl_ranks'] == 2


# (world 8 on one device: opt-in, MMNAS_TEST_WORLD8=1 -- see tests/test_dp_gpu.py)
@pytest.mark.parametrize('workload,world', [('train_vqa', 2), ('search_vqa', 2), ('bilevel_vqa', 2), ('search_vqa', 4), ('bilevel_vqa', 4)]
                         + ([('search_vqa', 8)] if os.environ.get('MMNAS_TEST_WORLD8') == '1' else []))
def test_bench_two_ranks_one_gpu(workload, world, tmp_path):
    """N ranks on the box's ONE GPU over gloo (RCCL refuses two ranks on a device), launched exactly as the driver launches
    N > 1.  world 4 / 8 (round 6): the N > 2 branches of the harness -- rank counting, architecture comparison, per-rank
    times, and the persistent LSTM with 4 / 8 processes' grids sharing the CUs: either every hand-off is met
    (`lstm_timed_out` 0) or EVERY rank fell back to nn.LSTM together (`lstm_fallback`), never a hang or a NaN loss."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MMNAS_BENCH_BACKEND='gloo', MMNAS_BENCH_DEVICE='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
                        '--master-addr', '127.0.0.1', '--master-port', str(port), 'bench.py', '--gpus', str(world),
                        '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--workload', workload, '--full-out', str(tmp_path / 'f.json')],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    d = _json_line(p.stdout, str(tmp_path / 'f.json'))
    if workload == 'bilevel_vqa':
        _check(d, world, steps=6, warmup=6)
    else:
        _check(d, world)
    assert d['config']['parallelism'] == 'dp%d' % world and d['config']['grad_allreduce'] == 'gloo'
    # what the line says about the exchange is observed in the run: ranks counted by an all-reduce, the ranks' sampled
    # architectures compared before the timed blocks, the LSTM hand-off flag read after every block, each rank's own time
    c = d['config']
    assert c['rccl_ranks'] == world and c['rank_id_sum_ok'] is True
    # 2 ranks: the two persistent grids are co-resident; more: a time-out is legitimate, but then all ranks fell back together
    assert c['lstm_timed_out'] == 0 and (world > 2 or c['lstm_fallback'] is False), (c['lstm_timed_out'], c['lstm_fallback'])
    assert c['dp_rows'] in ('0', '1')
    if workload != 'train_vqa':
        assert c['same_architecture'] is True and c['dp_buckets'] == 3
    full = json.load(open(str(tmp_path / 'f.json')))
    assert len(full['rank_ms_per_step']) == world and max(full['rank_ms_per_step']) == pytest.approx(full['ms_per_step'], rel=1e-3)
    assert len(d['rank_ms_per_step']) == world
