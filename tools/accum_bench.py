"""What micro-batch gradient accumulation costs (profiles/accum/README.md).  One process, one device:

  kernel    ops.grad_accumulate in each mode on a ResNet-50-sized arena (25 502 912 fp32), HIP events around each of --reps
            calls, next to a device-to-device copy of the same arena timed the same way.  Every call works on the next of
            --ring buffer pairs, so no call finds its operands in the 256 MiB last-level cache -- as in a training step, where
            a whole forward and backward pass lies between two passes over the arena.
  wrn22     bench.py's WRN-22 configuration at batch 128 under train.GraphedStep: the plain step (no MicroBatches: what the
            parent commit runs) and train.MicroBatches with k = 1, 2, 4, 8, each on a graph of its own, timed in alternating
            blocks (host clock around a device synchronise); median images/s and milliseconds per micro-batch over --rounds
  resnet50  bench.py's ResNet-50 configuration at batch 128, eager, the same arms

Writes <out>/accum_bench.jsonl and <out>/tables.md (the tables of the README).
Usage: python tools/accum_bench.py [--rounds 5] [--reps 40] [--ring 4] [--skip kernel,wrn22,resnet50] [--out profiles/accum]
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
ARENA = 25502912
KS = (1, 2, 4, 8)


def bench_kernel(args):
  from rigl_amd import _lib, ops
  pairs = [(torch.randn(ARENA, device=DEV), torch.randn(ARENA, device=DEV)) for _ in range(args.ring)]
  la, lm, l = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
  turn = [0]

  def timed(fn):
    ms = []
    for i in range(args.reps + 5):
      a, g = pairs[turn[0] % len(pairs)]
      turn[0] += 1
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn(a, g)
      e1.record()
      e1.synchronize()
      if i >= 5:
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]
  arms = [('copy', 2, lambda a, g: a.copy_(g)),
          ('first', 2, lambda a, g: ops.grad_accumulate(a, g, _lib.ACC_FIRST, loss=l, loss_acc=la)),
          ('add', 3, lambda a, g: ops.grad_accumulate(a, g, _lib.ACC_ADD, loss=l, loss_acc=la)),
          ('last', 3, lambda a, g: ops.grad_accumulate(a, g, _lib.ACC_LAST, loss=l, loss_acc=la, loss_mean=lm, inv_k=0.25)),
          ('copy_again', 2, lambda a, g: a.copy_(g))]
  out = {'what': 'kernel', 'elements': ARENA, 'reps': args.reps, 'ring_pairs': args.ring}
  for name, streams, fn in arms:
    med, lo, hi = timed(fn)
    nbytes = streams * ARENA * 4
    out[name] = {'streams': streams, 'bytes': nbytes, 'us_median': round(med * 1e3, 1), 'us_min': round(lo * 1e3, 1),
                 'us_max': round(hi * 1e3, 1), 'TBps_median': round(nbytes / med / 1e9, 3), 'TBps_best': round(nbytes / lo / 1e9, 3)}
  print(json.dumps(out), flush=True)
  return out


def build(workload, batch, k, graphed):
  """k None: the plain step, no MicroBatches anywhere."""
  import bench
  from rigl_amd import sparse_optimizers as SO, train, variables as V
  g = V.Graph(DEV)
  wl = bench.build_workload(workload, g, torch.device(DEV), batch, 0, None)
  inner = train.MomentumOptimizer(wl['lr'](batch), 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, grow_init='zeros', initial_acc_scale=0.0, **wl['opt'])
  gs = g.get_or_create_global_step()
  fn = wl['loss'] if k is None else train.MicroBatches(wl['loss'], opt, micro_batches=k)
  if graphed:
    step = train.GraphedStep(fn, opt, gs)
  else:
    def step():
      loss = fn()
      opt.minimize(loss, gs)
      return loss
  return dict(step=step, gs=gs, k=k or 1, graphed=graphed)


def bench_steps(workload, batch, graphed, args, micro_per_block, warmup):
  arms = {'plain': build(workload, batch, None, graphed)}
  for k in KS:
    arms['k%d' % k] = build(workload, batch, k, graphed)
  for r in arms.values():
    for _ in range(warmup):
      r['step']()
  torch.cuda.synchronize()
  secs = {a: [] for a in arms}
  for _ in range(args.rounds):
    for a, r in arms.items():
      block = max(micro_per_block // r['k'], 1)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(block):
        r['step']()
      torch.cuda.synchronize()
      secs[a].append((time.perf_counter() - t0) / (block * r['k']))          # seconds per micro-batch
  out = {'what': 'step', 'workload': workload, 'micro_batch': batch, 'mode': 'graph replay' if graphed else 'eager',
         'micro_batches_per_block': micro_per_block, 'rounds': args.rounds}
  for a, r in arms.items():
    v = sorted(secs[a])
    med = v[len(v) // 2]
    out[a] = {'k': r['k'], 'images_per_s_median': round(batch / med, 1), 'images_per_s_min': round(batch / v[-1], 1),
              'images_per_s_max': round(batch / v[0], 1), 'ms_per_micro_batch_median': round(med * 1e3, 4),
              'ms_per_micro_batch_min': round(v[0] * 1e3, 4), 'ms_per_micro_batch_max': round(v[-1] * 1e3, 4),
              'global_step': int(r['gs'].value)}
    if graphed:
      out[a].update(replays=r['step'].replays, eager_steps=r['step'].eager_steps)
  print(json.dumps(out), flush=True)
  return out


def tables(rows):
  L = []
  for r in rows:
    if r['what'] == 'kernel':
      L += ['| | arena streams | bytes | median | min - max | median rate | best rate |', '|---|---|---|---|---|---|---|']
      for name in ('copy', 'first', 'add', 'last', 'copy_again'):
        a = r[name]
        L.append('| %s | %d | %d | %.1f us | %.1f - %.1f us | %.3f TB/s | %.3f TB/s |' % (
            name, a['streams'], a['bytes'], a['us_median'], a['us_min'], a['us_max'], a['TBps_median'], a['TBps_best']))
      L.append('')
    if r['what'] == 'step':
      L += ['%s, micro-batch %d, %s:' % (r['workload'], r['micro_batch'], r['mode']), '',
            '| arm | images/s median (min - max) | ms per micro-batch median (min - max) | over plain |', '|---|---|---|---|']
      for name in ['plain'] + ['k%d' % k for k in KS]:
        a = r[name]
        L.append('| %s | %s (%s - %s) | %.4f (%.4f - %.4f) | %.4f |' % (
            name, a['images_per_s_median'], a['images_per_s_min'], a['images_per_s_max'], a['ms_per_micro_batch_median'],
            a['ms_per_micro_batch_min'], a['ms_per_micro_batch_max'],
            a['images_per_s_median'] / r['plain']['images_per_s_median']))
      L.append('')
  return '\n'.join(L)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=40)
  ap.add_argument('--ring', type=int, default=4)
  ap.add_argument('--skip', default='')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accum'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('accum_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  box = {'what': 'box', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'lib_sha16': sha}
  print(json.dumps(box), flush=True)
  skip = set(args.skip.split(','))
  rows = [box]
  if 'kernel' not in skip:
    rows.append(bench_kernel(args))
  if 'wrn22' not in skip:
    rows.append(bench_steps('wrn22', 128, True, args, micro_per_block=80, warmup=12))
  if 'resnet50' not in skip:
    rows.append(bench_steps('resnet50', 128, False, args, micro_per_block=16, warmup=4))
  os.makedirs(args.out, exist_ok=True)
  with open(os.path.join(args.out, 'accum_bench.jsonl'), 'w') as fh:
    for r in rows:
      fh.write(json.dumps(r) + '\n')
  with open(os.path.join(args.out, 'tables.md'), 'w') as fh:
    fh.write(tables(rows))


if __name__ == '__main__':
  main()
