"""What the per-step training summaries cost (profiles/summaries/README.md).  One process, one device:

  wrn22     bench.py's WRN-22 configuration at batch 128 under train.GraphedStep, two optimizers on graphs of their own -- one
            with rigl_amd.summaries.TrainingSummaries attached, one without (the parent commit's line) -- timed in alternating
            blocks (host clock around a device synchronise), median images/s over --rounds
  resnet50  bench.py's ResNet-50 configuration at batch 128, eager, the same pair
  pass      ops.summary_step alone on the ResNet-50 table (every trainable variable; 8 B per element plus the bitmaps), HIP
            events around --reps calls, next to a device-to-device copy of as many bytes as the pass reads

Writes profiles/summaries/summaries_bench.jsonl and profiles/summaries/README.md.
Usage: python tools/summaries_bench.py [--rounds 7] [--skip wrn22,resnet50,pass] [--out profiles/summaries]
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


def build(workload, batch, attach, graphed):
  import bench
  from rigl_amd import sparse_optimizers as SO, summaries, train, variables as V
  g = V.Graph(DEV)
  wl = bench.build_workload(workload, g, torch.device(DEV), batch, 0, None)
  inner = train.MomentumOptimizer(wl['lr'](batch), 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, grow_init='zeros', initial_acc_scale=0.0, **wl['opt'])
  gs = g.get_or_create_global_step()
  loss_fn = wl['loss']
  summ = summaries.TrainingSummaries(g, opt, ring=256).attach() if attach else None
  if graphed:
    step = train.GraphedStep(loss_fn, opt, gs)
  else:
    def step():
      loss = loss_fn()
      opt.minimize(loss, gs)
      return loss
  return dict(g=g, step=step, summ=summ, gs=gs, graphed=graphed)


def bench_pair(workload, batch, graphed, args, block, warmup):
  runs = {'without': build(workload, batch, False, graphed), 'with': build(workload, batch, True, graphed)}
  for r in runs.values():
    for _ in range(warmup):
      r['step']()
  torch.cuda.synchronize()
  rates = {a: [] for a in runs}
  records = dropped = 0
  for _ in range(args.rounds):
    for a, r in runs.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(block):
        r['step']()
      torch.cuda.synchronize()
      rates[a].append(batch * block / (time.perf_counter() - t0))
      if r['summ'] is not None:                       # read outside the timed block, as a logging loop would every N steps
        recs, d = r['summ'].read()
        records, dropped, last = records + len(recs), dropped + d, recs[-1]
  out = {'what': 'step', 'workload': workload, 'batch': batch, 'mode': 'graph replay' if graphed else 'eager',
         'block_steps': block, 'rounds': args.rounds, 'records_read': records, 'records_dropped': dropped,
         'last_record': {k: v for k, v in last.items() if not k.startswith('pruning/')}}
  for a, r in runs.items():
    v = sorted(rates[a])
    out[a] = {'images_per_s_median': round(v[len(v) // 2], 1), 'min': round(v[0], 1), 'max': round(v[-1], 1),
              'global_step': int(r['gs'].value)}
    if graphed:
      out[a].update(replays=r['step'].replays, eager_steps=r['step'].eager_steps)
  out['with_over_without'] = round(out['with']['images_per_s_median'] / out['without']['images_per_s_median'], 4)
  out['entries'] = len(runs['with']['summ'].layout)
  print(json.dumps(out), flush=True)
  return out, runs['with']


def bench_pass(run, args):
  from rigl_amd import ops
  summ = run['summ']
  table = summ._tables[False]                          # pylint: disable=protected-access
  n = sum(l['n'] for l in summ.layout)
  mask_bytes = sum((l['n'] + 31) // 32 * 4 for l in summ.layout if l['mask'])
  nbytes = 8 * n + mask_bytes
  step = torch.zeros(1, dtype=torch.int32, device=DEV)
  ring = torch.zeros(4 * ops.summary_slot_bytes(len(summ.layout)), dtype=torch.uint8, device=DEV)
  src = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
  dst = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

  def timed(fn):
    for _ in range(5):
      fn()
    ms = []
    for _ in range(args.reps):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      b.synchronize()
      ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]
  p = timed(lambda: ops.summary_step(table, step, ring, 4, lr=0.1))
  c = timed(lambda: dst.copy_(src))
  out = {'what': 'pass', 'table': 'resnet50', 'entries': len(summ.layout), 'elements': n, 'bytes_read': nbytes,
         'bytes_per_element': round(nbytes / n, 3), 'launches': -(-len(summ.layout) // 64) + 1,
         'pass_us_median': round(p[0] * 1e3, 1), 'pass_us_min': round(p[1] * 1e3, 1), 'pass_us_max': round(p[2] * 1e3, 1),
         'pass_read_GBps': round(nbytes / p[0] / 1e6, 1),
         'copy_us_median': round(c[0] * 1e3, 1), 'copy_us_min': round(c[1] * 1e3, 1), 'copy_us_max': round(c[2] * 1e3, 1),
         'copy_read_plus_write_GBps': round(2 * nbytes / c[0] / 1e6, 1), 'reps': args.reps}
  print(json.dumps(out), flush=True)
  return out


def readme(box, rows):
  L = ['# Per-step training summaries: what they cost', '',
       'One %s, torch %s, `librigl_hip.so` sha256[:16] `%s`.  `python tools/summaries_bench.py` wrote `summaries_bench.jsonl`'
       % (box['device'], box['torch'], box['lib_sha16']),
       'in one process.  Each step pair is two optimizers on graphs of their own, one with `TrainingSummaries` attached (ring of',
       '256 slots, read once per block outside the timed region) and one without -- the parent commit\'s line -- timed in',
       'alternating blocks, host clock around a device synchronise, median images/s per arm.  No speed gate: the figures are',
       'recorded, not promised.', '', '## Step', '',
       '| workload | mode | without: images/s median (min - max) | with: images/s median (min - max) | with / without | entries | records read / dropped |',
       '|---|---|---|---|---|---|---|']
  for r in rows:
    if r['what'] != 'step':
      continue
    f = lambda a: '%s (%s - %s)' % (r[a]['images_per_s_median'], r[a]['min'], r[a]['max'])
    L.append('| %s, batch %d | %s | %s | %s | **%.4f** | %d | %d / %d |' % (
        r['workload'], r['batch'], r['mode'], f('without'), f('with'), r['with_over_without'], r['entries'], r['records_read'],
        r['records_dropped']))
  for r in rows:
    if r['what'] == 'pass':
      L += ['', '## The pass alone', '',
            '`ops.summary_step` on the ResNet-50 table: %d entries, %d elements, %d bytes read (%.3f B / element: two fp32'
            % (r['entries'], r['elements'], r['bytes_read'], r['bytes_per_element']),
            'arenas and the bitmaps of the masked kernels), %d launches; HIP events around each of %d calls.' % (r['launches'], r['reps']),
            '', '| | median | min - max | traffic |', '|---|---|---|---|',
            '| summary pass | %.1f us | %.1f - %.1f us | %.1f GB/s read |' % (r['pass_us_median'], r['pass_us_min'], r['pass_us_max'], r['pass_read_GBps']),
            '| device copy of the same %d bytes | %.1f us | %.1f - %.1f us | %.1f GB/s read + write |'
            % (r['bytes_read'], r['copy_us_median'], r['copy_us_min'], r['copy_us_max'], r['copy_read_plus_write_GBps'])]
  L += ['', '## Parity', '',
        '`tests/test_summary_gpu.py` holds the pass to `tests/summary_ref.py` (integer outputs exact, fp64 sums within',
        '2 n 2^-53 of the exactly rounded value, bits independent of the grid, the run and the workspace\'s contents);',
        '`tests/test_summary_step_gpu.py` holds eager and replayed records bit-identical and the training run itself bit-identical',
        'with and without summaries attached.', '']
  return '\n'.join(L)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--skip', default='')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'summaries'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('summaries_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  box = {'what': 'box', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
         'lib_sha16': sha}
  print(json.dumps(box), flush=True)
  skip = set(args.skip.split(','))
  rows = [box]
  if 'wrn22' not in skip:
    rows.append(bench_pair('wrn22', 128, True, args, block=100, warmup=30)[0])
  if 'resnet50' not in skip:
    out, run = bench_pair('resnet50', 128, False, args, block=30, warmup=8)
    rows.append(out)
    if 'pass' not in skip:
      rows.append(bench_pass(run, args))
  os.makedirs(args.out, exist_ok=True)
  with open(os.path.join(args.out, 'summaries_bench.jsonl'), 'w') as fh:
    for r in rows:
      fh.write(json.dumps(r) + '\n')
  with open(os.path.join(args.out, 'README.md'), 'w') as fh:
    fh.write(readme(box, rows))


if __name__ == '__main__':
  main()
