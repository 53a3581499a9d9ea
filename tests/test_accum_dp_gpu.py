"""train.MicroBatches combined with the data-parallel exchange (dist.GradSync): one exchange per optimizer step, started inside
the k-th backward pass.  Subprocesses run tests/accum_dp_worker.py (fresh ports from 29601); a model's worker runs once per
module and the tests below read its report.

Models: the MNIST MLP at batch 32 (bucket 4 KiB: three kernel buckets and the flush) and a WideResNet of two blocks per group on
8 x 8 images at batch 16 (every conv masked, so that backward walks the arena from its end; bucket 64 KiB; a BN / bias segment
of 13 batch norms).  Global steps 0 and 2 are mask updates.

  one rank, exchange forced on, gloo, k = 3   W, the mask bitmap, the slots and G after each of five calls are bit-identical to
                                              the run with grad_sync=None: every element got LAST exactly once
  two ranks on cuda:0, gloo, k = 2            after call 0's compute_gradients G == fl(S_0 + S_1) bit for bit on both ranks
                                              (S_r: the arena of a no-exchange MicroBatches(k = 2) on rank r's micro-batches);
                                              identical masks after every call
  two ranks x k = 2 against one rank x k = 4  both models, on the same four micro-batches per call: equal global step and
                                              per-layer mask counts, and the tolerances of tests/test_dp_two_gpu.py (first loss
                                              1e-6 relative, later losses 1e-4, weight norm 1e-5).  Batch norm is per pass in
                                              both runs, so the WideResNet's two runs see the same batch statistics; what differs
                                              is the order of the fp32 additions over the four micro-gradients
  collectives (torch.distributed.all_reduce wrapped in the worker): none before the k-th pass; per call as many as a plain
  data-parallel step of the model at that bucket size; timeline bytes == 4 * G.numel()
  k == 1 with an exchange                     the kernel launches of a plain data-parallel step, no accumulate launch, no arena
  the two-rank cases over RCCL on two devices skipped where fewer than two GPUs are visible
"""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'accum_dp_worker.py')
N_DEV = torch.cuda.device_count() if torch.cuda.is_available() else 0
two_gpus = pytest.mark.skipif(N_DEV < 2, reason='needs two GPUs (found %d)' % N_DEV)
PORTS = {('forced', 'mlp'): 29601, ('forced', 'wrn'): 29602, ('two', 'mlp', 'gloo'): 29603, ('two', 'wrn', 'gloo'): 29604,
         ('two', 'mlp', 'nccl'): 29605, ('two', 'wrn', 'nccl'): 29606}
CALLS = 5
_REPORTS = {}


def _env():
  env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
  for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
    env.pop(k, None)
  return env


def _report(tmp_path_factory, *key):
  if key not in _REPORTS:
    out = str(tmp_path_factory.mktemp('accum_dp') / ('_'.join(key) + '.json'))
    port = PORTS[key]
    if key[0] == 'forced':
      cmd = [sys.executable, WORKER, '--case', 'forced', '--model', key[1], '--port', str(port), '--out', out]
    else:
      cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
             '--master-port', str(port), WORKER, '--case', 'two', '--model', key[1], '--backend', key[2], '--out', out]
    run = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    with open(out) as fh:
      _REPORTS[key] = json.load(fh)
  return _REPORTS[key]


MODELS = pytest.mark.parametrize('model', ['mlp', 'wrn'])


# ---- one rank, the exchange forced on ------------------------------------------------------------------------------------------
@MODELS
def test_forced_exchange_leaves_the_bits_of_the_run_without_one(tmp_path_factory, model):
  r = _report(tmp_path_factory, 'forced', model)
  assert r['world'] == 1 and r['backend'] == 'gloo' and r['enabled'] is True and r['grad_scale'] == 1.0 and r['k'] == 3
  a, b = r['exchange'], r['alone']
  assert len(a) == len(b) == CALLS
  for s, (x, y) in enumerate(zip(a, b)):
    for key in ('W', 'BITS', 'slot', 'G', 'gs', 'loss'):
      assert x[key] == y[key], (s, key)
  assert [x['gs'] for x in a] == [0, 1, 2, 2, 3]                      # calls 0 and 3 are the mask updates of steps 0 and 2
  assert len({x['W'] for x in a}) >= 4 and len({x['BITS'] for x in a}) == 2 and len({x['G'] for x in a}) == CALLS
  # without an exchange: two whole-arena passes and the whole-arena LAST; with one: the LAST pass rides with the buckets
  for x, y in zip(a, b):
    assert y['accumulate'] == 3 and y['accumulate_ranges'] == 0 and y['all_reduce'] == 0
    # (one ranges launch per bucket and ONE for the flush, whose two ranges gloo sends as two collectives)
    assert x['accumulate'] == 2 and 3 <= x['launches'] - 1 <= x['accumulate_ranges'] <= x['launches']


@MODELS
def test_forced_exchange_collectives(tmp_path_factory, model):
  r = _report(tmp_path_factory, 'forced', model)
  plain = r['plain']['calls']
  assert all(p['all_reduce'] == plain[0]['all_reduce'] >= 4 for p in plain)
  for x in r['exchange']:
    assert x['passes'] == 3 and x['held'] == 0                       # nothing is exchanged before the k-th pass begins
    assert x['all_reduce'] == plain[0]['all_reduce']                 # one exchange: the collectives of a plain step
    assert x['timeline_bytes'] == x['arena_bytes'] > 0               # every element of G exchanged exactly once
    assert x['launches'] >= 3
  for p in plain:
    assert p['timeline_bytes'] == p['arena_bytes']


@MODELS
def test_one_micro_batch_with_an_exchange_is_a_plain_data_parallel_step(tmp_path_factory, model):
  r = _report(tmp_path_factory, 'forced', model)
  plain, k1 = r['plain'], r['k1']
  assert k1['launches'] == plain['launches'] and sum(plain['launches'].values()) > 3
  for p, q in zip(plain['calls'], k1['calls']):
    assert q['accumulate'] == q['accumulate_ranges'] == 0 == p['accumulate'] == p['accumulate_ranges']
    assert q['all_reduce'] == p['all_reduce'] and q['timeline_bytes'] == p['timeline_bytes'] and q['launches'] == p['launches']
  assert k1['arena'] is True                                          # no second arena was allocated
  assert k1['digests'] == plain['digests']


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _check_two_ranks(r, backend):
  assert r['world'] == 2 and r['backend'] == backend and r['k'] == 2
  assert r['S_differ'] > 0                                            # the two ranks' sums are different gradients
  assert r['g_words'] > 0 and r['g_words_differing_from_fl_S0_plus_S1'] == 0
  assert r['update_scale'] == 0.25                                    # 1 / world x 1 / k, in one place
  assert r['masks_identical'] == [True] * CALLS
  plain = r['plain_calls']
  assert all(p['all_reduce'] == plain[0]['all_reduce'] for p in plain)
  for x in r['calls']:
    assert x['passes'] == 2 and x['held'] == 0
    assert x['all_reduce'] == plain[0]['all_reduce']
    assert x['timeline_bytes'] == x['arena_bytes'] > 0 and x['launches'] >= 3
    assert x['accumulate'] == 1 and x['launches'] - 1 <= x['accumulate_ranges'] <= x['launches']
  assert [x['gs'] for x in r['calls']] == [0, 1, 2, 2, 3]


@MODELS
def test_two_ranks_sum_their_sums_gloo(tmp_path_factory, model):
  _check_two_ranks(_report(tmp_path_factory, 'two', model, 'gloo'), 'gloo')


def _check_two_by_two_is_one_by_four(r):
  two, one = r['two'], r['one']
  assert two['global_step'] == one['global_step'] == 3 and two['mask_ones'] == one['mask_ones']
  a, b = [x['loss'] for x in r['calls']], one['losses']
  print('accum dp: losses two x 2 %r, one x 4 %r; weight norms %r %r' % (a, b, two['w_norm'], one['w_norm']))
  assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]), (a, b)
  for x, y in zip(a, b):
    assert abs(x - y) <= 1e-4 * max(abs(y), 1.0), (a, b)
  assert abs(two['w_norm'] - one['w_norm']) <= 1e-5 * one['w_norm']


@MODELS
def test_two_ranks_of_two_equal_one_rank_of_four_gloo(tmp_path_factory, model):
  _check_two_by_two_is_one_by_four(_report(tmp_path_factory, 'two', model, 'gloo'))


@two_gpus
@MODELS
def test_two_ranks_sum_their_sums_rccl(tmp_path_factory, model):
  _check_two_ranks(_report(tmp_path_factory, 'two', model, 'nccl'), 'nccl')


@two_gpus
@MODELS
def test_two_ranks_of_two_equal_one_rank_of_four_rccl(tmp_path_factory, model):
  _check_two_by_two_is_one_by_four(_report(tmp_path_factory, 'two', model, 'nccl'))
