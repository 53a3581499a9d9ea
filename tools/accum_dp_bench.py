"""What micro-batch accumulation costs once it is combined with the data-parallel exchange (profiles/accum_dp/README.md).
One process, ONE device, the ResNet-50 arena of bench.py's default workload:

  flush     the final flush of an accumulated data-parallel step -- the head of the kernel segment left over by the buckets and
            the BN / bias segment -- as ONE ops.grad_accumulate_ranges(LAST) launch with the loss arithmetic, against two plain
            ops.grad_accumulate(LAST) launches over the same two ranges (the second with the loss arithmetic)
  buckets   the LAST pass of every exchange bucket at --bucket-mb (default: GradSync's 32 MB), each launch timed on its own,
            and their sum, against the ONE whole-arena LAST launch a step without an exchange runs (the parent commit's pass)
  step      a k = 4 ResNet-50 step at micro-batch 128 with a ONE-rank exchange forced on (RCCL, world 1: the whole machinery
            -- held passes, per-bucket LAST, collectives, flush -- with nothing on the wire) against the same step without a
            GradSync (the parent commit's accumulated step), in alternating blocks

The kernel arms take HIP events around each of --reps calls after 5 untimed ones; every call works on the next of --ring arena
pairs, so no call finds its operands in the last-level cache.  What a multi-GPU node would show -- how much of the exchange
the k-th backward pass hides -- cannot be measured on one device and is not estimated here.

Writes <out>/accum_dp_bench.jsonl and <out>/README.md.
Usage: python tools/accum_dp_bench.py [--rounds 5] [--reps 40] [--ring 4] [--bucket-mb 32] [--skip flush,buckets,step]
                                      [--out profiles/accum_dp]

Kernel time without the launch gap an event pair includes comes from a kernel trace of the two kernel arms:
  rocprofv3 --kernel-trace -d DIR -o acc -- python tools/accum_dp_bench.py --skip step --out SOMEWHERE_ELSE
  python tools/accum_dp_bench.py --trace-db DIR/.../acc_results.db --out profiles/accum_dp
The second call measures nothing: it assigns the traced dispatches of the two accumulate kernels to the arms by kernel, grid and
call order (the arms' launches are known from the recorded rows), adds the `trace` row to <out>/accum_dp_bench.jsonl, writes
<out>/kernel_trace.csv and rewrites the README with both sets of figures.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = 'cuda:0'
K = 4
BATCH = 128


def arena_layout(bucket_mb):
  """The ResNet-50 arena of bench.py: elements, the end of the kernel segment, and the ranges a data-parallel step sends, in
  launch order -- what GradSync cuts when backward produces the kernel gradients from the arena's end to its start."""
  import bench
  from rigl_amd import variables as V
  g = V.Graph(DEV)
  bench.build_workload('resnet50', g, torch.device(DEV), 8, 0, None)
  g.finalize()
  kend, end = g.seg[V.KIND_DENSE][1], g.G.numel()
  elems = max(int(bucket_mb * (1 << 20)) // 4, 1)
  offs = sorted(v.offset for v in g.trainable_variables() if v.kind in (V.KIND_MASKED, V.KIND_DENSE))
  buckets, hi = [], kend
  for lo in reversed(offs):
    if hi - lo >= elems:
      buckets.append((lo, hi))
      hi = lo
  flush = [(lo, h) for lo, h in ((0, hi), (kend, end)) if h > lo]
  return dict(elements=end, kernel_end=kend, buckets=buckets, flush=flush)


def _stats(ms):
  ms = sorted(ms)
  return {'us_median': round(ms[len(ms) // 2] * 1e3, 2), 'us_min': round(ms[0] * 1e3, 2), 'us_max': round(ms[-1] * 1e3, 2)}


class Kernels:

  def __init__(self, n, args):
    self.pairs = [(torch.randn(n, device=DEV), torch.randn(n, device=DEV)) for _ in range(args.ring)]
    self.la, self.lm, self.l = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    self.reps, self.turn = args.reps, 0
    self.loss = dict(loss=self.l, loss_acc=self.la, loss_mean=self.lm, inv_k=1.0 / K)

  def timed(self, fn):
    ms = []
    for i in range(self.reps + 5):
      a, g = self.pairs[self.turn % len(self.pairs)]
      self.turn += 1
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn(a, g)
      e1.record()
      e1.synchronize()
      if i >= 5:
        ms.append(e0.elapsed_time(e1))
    return ms


def bench_flush(lay, kern):
  from rigl_amd import _lib, ops
  flush = lay['flush']
  spans = [(lo, hi - lo) for lo, hi in flush]

  def ranges(a, g):
    ops.grad_accumulate_ranges(a, g, spans, _lib.ACC_LAST, **kern.loss)

  def plain(a, g):
    for i, (lo, hi) in enumerate(flush):
      ops.grad_accumulate(a[lo:hi], g[lo:hi], _lib.ACC_LAST, **(kern.loss if i == len(flush) - 1 else {}))
  out = {'what': 'flush', 'ranges': flush, 'bytes': 3 * 4 * sum(n for _, n in spans), 'reps': kern.reps}
  for name, fn in (('plain_launches', plain), ('ranges_launch', ranges), ('plain_launches_again', plain),
                   ('ranges_launch_again', ranges)):
    out[name] = _stats(kern.timed(fn))
  print(json.dumps(out), flush=True)
  return out


def bench_buckets(lay, kern, bucket_mb):
  from rigl_amd import _lib, ops
  n = lay['elements']
  out = {'what': 'buckets', 'bucket_mb': bucket_mb, 'elements': n, 'reps': kern.reps, 'per_bucket': []}
  whole = lambda a, g: ops.grad_accumulate(a, g, _lib.ACC_LAST, **kern.loss)
  out['whole_arena_last'] = _stats(kern.timed(whole))
  sums = [0.0] * kern.reps
  parts = [[(lo, hi)] for lo, hi in lay['buckets']] + [lay['flush']]
  for i, part in enumerate(parts):
    spans = [(lo, hi - lo) for lo, hi in part]
    kw = kern.loss if i == len(parts) - 1 else {}
    ms = kern.timed(lambda a, g, spans=spans, kw=kw: ops.grad_accumulate_ranges(a, g, spans, _lib.ACC_LAST, **kw))
    out['per_bucket'].append(dict(_stats(ms), ranges=part, elements=sum(m for _, m in spans)))
    sums = [s + m for s, m in zip(sums, sorted(ms))]                 # i-th fastest of every bucket together
  out['bucket_launches'] = len(parts)
  out['sum_of_bucket_lasts'] = _stats(sums)
  out['sum_of_bucket_medians_us'] = round(sum(b['us_median'] for b in out['per_bucket']), 2)
  out['whole_arena_last_again'] = _stats(kern.timed(whole))
  assert sum(b['elements'] for b in out['per_bucket']) == n
  print(json.dumps(out), flush=True)
  return out


def build_step(exchange, bucket_mb):
  import bench
  from rigl_amd import sparse_optimizers as SO, train, variables as V
  from rigl_amd.dist import GradSync
  g = V.Graph(DEV)
  wl = bench.build_workload('resnet50', g, torch.device(DEV), BATCH, 0, None)
  sync = GradSync(g, bucket_bytes=int(bucket_mb * (1 << 20)), enabled=True) if exchange else None
  inner = train.MomentumOptimizer(wl['lr'](BATCH), 0.9, use_nesterov=True, graph=g, grad_sync=sync)
  opt = SO.SparseRigLOptimizer(inner, grow_init='zeros', initial_acc_scale=0.0, use_tpu=exchange, **wl['opt'])
  gs = g.get_or_create_global_step()
  mb = train.MicroBatches(wl['loss'], opt, micro_batches=K)

  def step():
    opt.minimize(mb(), gs)
  return dict(step=step, gs=gs, sync=sync)


def bench_step(args):
  import torch.distributed as dist
  os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
  os.environ.setdefault('MASTER_PORT', '29611')
  os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  dist.init_process_group('nccl', device_id=torch.device(DEV), rank=0, world_size=1)
  arms = {'k4_alone': build_step(False, args.bucket_mb), 'k4_one_rank_exchange': build_step(True, args.bucket_mb)}
  for r in arms.values():
    for _ in range(3):
      r['step']()
  torch.cuda.synchronize()
  secs = {a: [] for a in arms}
  for _ in range(args.rounds):
    for a, r in arms.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.steps_per_block):
        r['step']()
      torch.cuda.synchronize()
      secs[a].append((time.perf_counter() - t0) / args.steps_per_block)
  out = {'what': 'step', 'workload': 'resnet50', 'micro_batch': BATCH, 'k': K, 'mode': 'eager', 'rounds': args.rounds,
         'steps_per_block': args.steps_per_block, 'backend': dist.get_backend(), 'world': 1, 'bucket_mb': args.bucket_mb}
  for a, r in arms.items():
    v = sorted(secs[a])
    med = v[len(v) // 2]
    out[a] = {'ms_per_step_median': round(med * 1e3, 3), 'ms_per_step_min': round(v[0] * 1e3, 3),
              'ms_per_step_max': round(v[-1] * 1e3, 3), 'images_per_s_median': round(K * BATCH / med, 1),
              'global_step': int(r['gs'].value)}
    if r['sync'] is not None:
      out[a]['collective_launches_per_step'] = r['sync'].n_buckets_last
  dist.destroy_process_group()
  print(json.dumps(out), flush=True)
  return out


def _grid(kernel, spans):
  """Workgroups of one launch: accumulate.hip's grid for a whole-arena pass ('acc') or a ranges pass ('rng') over ``spans``."""
  if kernel == 'acc':
    blocks = (spans[0][1] >> 2) // 1024
  else:
    blocks = -(-sum((n + 3) >> 2 for _, n in spans) // 1024)
  return max(min(blocks, 2048), 1)


def arm_plan(rows):
  """[(section, arm, [(kernel, workgroups) of every launch of one call])] in the order main() runs the kernel arms."""
  plan = []
  for r in rows:
    if r['what'] == 'flush':
      spans = [(lo, hi - lo) for lo, hi in r['ranges']]
      plain = [('acc', _grid('acc', [s])) for s in spans]
      for arm in ('plain_launches', 'ranges_launch', 'plain_launches_again', 'ranges_launch_again'):
        plan.append(('flush', arm, plain if arm.startswith('plain') else [('rng', _grid('rng', spans))]))
    if r['what'] == 'buckets':
      whole = [('acc', _grid('acc', [(0, r['elements'])]))]
      plan.append(('buckets', 'whole_arena_last', whole))
      for i, b in enumerate(r['per_bucket']):
        plan.append(('buckets', 'launch_%d' % i, [('rng', _grid('rng', [(lo, hi - lo) for lo, hi in b['ranges']]))]))
      plan.append(('buckets', 'whole_arena_last_again', whole))
  return plan


def trace_row(db, rows):
  """Kernel durations of every arm's timed calls from a rocprofv3 kernel trace of the run that main() makes with --skip step."""
  import sqlite3
  cur = sqlite3.connect(db).cursor()
  try:
    found = list(cur.execute('select name, grid_x, workgroup_x, duration from kernels order by start'))
  except sqlite3.OperationalError:
    found = list(cur.execute('select name, grid_x, workgroup_x, duration from kernels'))
  queues = {}
  for name, gx, wx, dur in found:
    kernel = 'rng' if 'k_accumulate_ranges' in name else 'acc' if 'k_accumulate' in name else None
    if kernel is not None:
      queues.setdefault((kernel, gx // wx), []).append(dur / 1e3)
  reps = next(r['reps'] for r in rows if r['what'] in ('flush', 'buckets'))
  out = {'what': 'trace', 'reps': reps, 'arms': [],
         'dispatches': {'%s@%d' % k: len(v) for k, v in sorted(queues.items())}}
  bucket_calls = []
  for section, arm, launches in arm_plan(rows):
    per_call = [0.0] * reps
    for key in launches:
      q = queues.get(key, [])
      if len(q) < reps + 5:
        raise SystemExit('accum_dp_bench: the trace holds %d dispatches of %s@%d where arm %s needs %d' %
                         (len(q), key[0], key[1], arm, reps + 5))
      mine, queues[key] = q[5:reps + 5], q[reps + 5:]            # the first 5 calls of an arm are untimed
      per_call = [a + b for a, b in zip(per_call, mine)]
    out['arms'].append(dict(_stats([v / 1e3 for v in per_call]), section=section, arm=arm,
                            launches=['%s@%d' % k for k in launches]))
    if arm.startswith('launch_'):
      bucket_calls.append(sorted(per_call))
  if bucket_calls:
    out['sum_of_bucket_lasts'] = _stats([sum(v) / 1e3 for v in zip(*bucket_calls)])
  left = {('%s@%d' % k): len(v) for k, v in queues.items() if v}
  if left:
    raise SystemExit('accum_dp_bench: the trace holds dispatches no arm accounts for: %r' % left)
  return out


def trace_csv(row, out_dir):
  with open(os.path.join(out_dir, 'kernel_trace.csv'), 'w') as fh:
    fh.write('section,arm,launches,calls,median_us,min_us,max_us\n')
    for a in row['arms']:
      fh.write('%s,%s,%s,%d,%.2f,%.2f,%.2f\n' % (a['section'], a['arm'], '+'.join(a['launches']), row['reps'], a['us_median'],
                                                 a['us_min'], a['us_max']))


def _row(name, s, t=None):
  tail = '' if t is None else ' %.2f us | %.2f - %.2f us |' % (t['us_median'], t['us_min'], t['us_max'])
  return '| %s | %.2f us | %.2f - %.2f us |%s' % (name, s['us_median'], s['us_min'], s['us_max'], tail)


def readme(rows):
  box = rows[0]
  trace = next((r for r in rows if r['what'] == 'trace'), None)
  t = {(a['section'], a['arm']): a for a in trace['arms']} if trace else {}
  head3 = '| median | min - max |' + (' kernel time, median | min - max |' if trace else '')
  rule3 = '|---|---|' + ('---|---|' if trace else '')
  L = ['# Micro-batch accumulation with the data-parallel exchange: what it costs on one GPU', '',
       'One %s (%s), torch %s, `librigl_hip.so` sha256[:16] `%s`.  `python tools/accum_dp_bench.py` wrote `accum_dp_bench.jsonl` and'
       % (box['device'], box['arch'], box['torch'], box['lib_sha16']),
       'this file.  No figure below was a gate decided in advance: they are recorded, not promised.  Everything is measured',
       'against what the parent commit runs -- its whole-arena `LAST` pass and its accumulated step without an exchange -- in the',
       'same process.  `bench.py` against the parent commit\'s tree is in `bench_ab.md`.', '',
       'The arena is ResNet-50\'s (`bench.py`\'s default workload): %d fp32, kernel segment `[0, %d)`, BN / bias segment behind it.'
       % (box['elements'], box['kernel_end']),
       'Kernel arms: HIP events around each call, 5 untimed calls first, every call on the next of %d arena pairs (cold operands).'
       % box['ring'],
       'An event pair around one launch includes the launch gap.']
  if trace:
    L += ['"Kernel time" is the duration of the same arms\' dispatches in a `rocprofv3 --kernel-trace` run of the two kernel arms',
          '(another process of the same session; `kernel_trace.csv`; a call of two launches counts both kernels, not the gap',
          'between them).']
  L.append('')
  for r in rows[1:]:
    if r['what'] == 'flush':
      L += ['## The final flush: one ranges launch against two plain launches', '',
            'Ranges %s (elements), `LAST` with the loss arithmetic, %d bytes read and written; %d timed calls per arm, the arms'
            % (' and '.join('`[%d, %d)`' % tuple(x) for x in r['ranges']), r['bytes'], r['reps']),
            'run twice in turn:', '', '| arm ' + head3, '|---' + rule3]
      for arm, name in (('plain_launches', 'two `ops.grad_accumulate` launches'),
                        ('ranges_launch', 'one `ops.grad_accumulate_ranges` launch'),
                        ('plain_launches_again', 'two launches, again'), ('ranges_launch_again', 'one ranges launch, again')):
        L.append(_row(name, r[arm], t.get(('flush', arm))))
      L.append('')
    if r['what'] == 'buckets':
      L += ['## The `LAST` pass bucket by bucket against the whole-arena pass', '',
            'Bucket size %s MB (`GradSync`\'s default is 32): %d launches per step, the last one the flush.  Each launch timed on'
            % (r['bucket_mb'], r['bucket_launches']),
            'its own (%d calls); "sum" adds the i-th fastest call of every launch:' % r['reps'], '',
            '| launch | elements ' + head3, '|---|---' + rule3]
      for i, b in enumerate(r['per_bucket']):
        L.append(_row('%s %s | %d' % ('flush' if i == len(r['per_bucket']) - 1 else 'bucket %d' % i,
                                      ' + '.join('`[%d, %d)`' % tuple(x) for x in b['ranges']), b['elements']),
                      b, t.get(('buckets', 'launch_%d' % i))))
      L += [_row('**sum of the launches** | %d' % r['elements'], r['sum_of_bucket_lasts'],
                 trace.get('sum_of_bucket_lasts') if trace else None),
            _row('whole-arena `LAST` (parent), before | %d' % r['elements'], r['whole_arena_last'],
                 t.get(('buckets', 'whole_arena_last'))),
            _row('whole-arena `LAST` (parent), after | %d' % r['elements'], r['whole_arena_last_again'],
                 t.get(('buckets', 'whole_arena_last_again'))), '']
      ev = r['sum_of_bucket_lasts']['us_median'] - r['whole_arena_last']['us_median']
      txt = ('As event pairs the %d launches of a step are %.1f us %s the one whole-arena launch (medians)'
             % (r['bucket_launches'], abs(ev), 'behind' if ev >= 0 else 'ahead of'))
      if trace and 'sum_of_bucket_lasts' in trace:
        kt = trace['sum_of_bucket_lasts']['us_median'] - t[('buckets', 'whole_arena_last')]['us_median']
        txt += ('; as kernel time %.1f us %s it (an event pair also holds its launch\'s gap, which the split pays %d times)'
                % (abs(kt), 'behind' if kt >= 0 else 'ahead of', r['bucket_launches']))
      L += [txt + '.', 'The launches were timed apart; in a step they lie between the backward kernels of the k-th pass.', '']
    if r['what'] == 'step':
      a, b = r['k4_alone'], r['k4_one_rank_exchange']
      d = b['ms_per_step_median'] - a['ms_per_step_median']
      spread = max(x['ms_per_step_max'] - x['ms_per_step_min'] for x in (a, b))
      L += ['## A k = %d step with a one-rank exchange forced on' % r['k'], '',
            'ResNet-50, micro-batch %d, eager, %d steps per block (about %.1f s), %d alternating rounds, host clock around a device'
            % (r['micro_batch'], r['steps_per_block'], r['steps_per_block'] * a['ms_per_step_median'] / 1e3, r['rounds']),
            'synchronise.  The exchange arm runs the whole machinery over RCCL with world 1 (%d collective launches per step at'
            % b.get('collective_launches_per_step', 0),
            '%s MB): held passes, a `LAST` launch per bucket, the collectives (with one rank nothing is sent), the flush.'
            % r['bucket_mb'], '',
            '| arm | ms per step median (min - max) | images/s median | over alone |', '|---|---|---|---|',
            '| k = %d, no `GradSync` (parent) | %.3f (%.3f - %.3f) | %.1f | 1.0000 |' % (
                r['k'], a['ms_per_step_median'], a['ms_per_step_min'], a['ms_per_step_max'], a['images_per_s_median']),
            '| k = %d, one-rank exchange | %.3f (%.3f - %.3f) | %.1f | %.4f |' % (
                r['k'], b['ms_per_step_median'], b['ms_per_step_min'], b['ms_per_step_max'], b['images_per_s_median'],
                b['images_per_s_median'] / a['images_per_s_median']), '',
            'The one-rank arm is %.3f ms per step (%.1f %%) %s the arm without a `GradSync`; the wider of the two arms\' min - max'
            % (abs(d), 100 * abs(d) / a['ms_per_step_median'], 'behind' if d >= 0 else 'ahead of'),
            'ranges is %.3f ms.  This run does not split that difference between the RCCL launches, their stream waits, the `LAST`'
            % spread,
            'launches (above) and the host work of the exchange, and a one-rank exchange is not what a multi-GPU step pays: there',
            'the collectives run on RCCL\'s stream beside the backward kernels.', '']
  L += ['## Not measured', '',
        'How much of the exchange the k-th backward pass hides on a multi-GPU node: one device has nothing on the wire, and a',
        'one-rank collective is no ring traversal.  No figure here stands in for it.  The evidence that the combined',
        'step is RIGHT on more than one rank is `tests/test_accum_dp_gpu.py` (two ranks over gloo on one device; the same cases over',
        'RCCL wherever two devices are visible), and the first multi-GPU node that runs `bench.py --gpus N` reports the exposed',
        'exchange time of a plain step as before.  `bench.py` runs no `MicroBatches`: nothing it enqueues has changed.', '']
  return '\n'.join(L)


def _write(out_dir, rows):
  os.makedirs(out_dir, exist_ok=True)
  with open(os.path.join(out_dir, 'accum_dp_bench.jsonl'), 'w') as fh:
    for r in rows:
      fh.write(json.dumps(r) + '\n')
  with open(os.path.join(out_dir, 'README.md'), 'w') as fh:
    fh.write(readme(rows))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=40)
  ap.add_argument('--ring', type=int, default=4)
  ap.add_argument('--bucket-mb', type=float, default=32.0)
  ap.add_argument('--steps-per-block', type=int, default=25)
  ap.add_argument('--skip', default='')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accum_dp'))
  ap.add_argument('--trace-db', default=None, help='measure nothing: add the kernel times of a rocprofv3 trace to <out>')
  args = ap.parse_args()
  if args.trace_db:
    with open(os.path.join(args.out, 'accum_dp_bench.jsonl')) as fh:
      rows = [r for r in map(json.loads, fh) if r['what'] != 'trace']
    rows.append(trace_row(args.trace_db, rows))
    trace_csv(rows[-1], args.out)
    _write(args.out, rows)
    return
  if not torch.cuda.is_available():
    raise SystemExit('accum_dp_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  lay = arena_layout(args.bucket_mb)
  box = {'what': 'box', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'lib_sha16': sha,
         'arch': getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?').split(':')[0],
         'elements': lay['elements'], 'kernel_end': lay['kernel_end'], 'ring': args.ring}
  print(json.dumps(box), flush=True)
  skip = set(args.skip.split(','))
  rows = [box]
  if not {'flush', 'buckets'} <= skip:
    kern = Kernels(lay['elements'], args)
    if 'flush' not in skip:
      rows.append(bench_flush(lay, kern))
    if 'buckets' not in skip:
      rows.append(bench_buckets(lay, kern, args.bucket_mb))
    del kern
    torch.cuda.empty_cache()
  if 'step' not in skip:
    rows.append(bench_step(args))
  _write(args.out, rows)


if __name__ == '__main__':
  main()
