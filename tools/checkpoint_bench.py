"""What an exact checkpoint costs (profiles/checkpoint/README.md).  One process, one device:

  kernel    ops.state_gather / ops.state_scatter on the region table of the ResNet-50 training state with Nesterov momentum
            (W, BITS, the momentum arena, 2 x 53 moving statistics), HIP events around each of --reps calls, next to
            torch.Tensor.copy_ of the same byte count timed the same way before and after.  Every call works on the next of
            --ring region sets and staging buffers, so no call finds its operands in the 256 MiB last-level cache.
  wrn22     bench.py's WRN-22 configuration at batch 128 under train.GraphedStep, three arms in alternating blocks of --block
            steps: no checkpoint; TrainingState.snapshot() every --every steps with Snapshot.save on a writer thread;
            tf_checkpoint.save_graph every --every steps (what the parent commit offers: an incomplete save, here only as the
            cost yardstick).  Also the stall of the training stream per snapshot (HIP events around the call) and the file size.

  snapshot  the host time of TrainingState.snapshot() on that ResNet-50 state (host clock around the call, the device idle in
            front of it), with the snapshot before it saved / released (nothing to move) and with it kept (a host copy of the
            208 MB image), and how long the copy-out to pinned memory then takes

Writes <out>/checkpoint_bench.jsonl and <out>/tables.md.  ``--trace DB``: instead of measuring, reads the database that
`rocprofv3 --kernel-trace -d DIR -o ck -- python tools/checkpoint_bench.py --skip wrn22,snapshot` left (DIR/ck_results.db)
and writes <out>/kernel_trace.csv: calls, median and minimum duration of the state kernels and of the copy kernel per grid.
Usage: python tools/checkpoint_bench.py [--rounds 5] [--reps 40] [--ring 3] [--block 200] [--every 50] [--skip kernel,snapshot,wrn22]
                                        [--out profiles/checkpoint] [--dir <where the files go>]
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = 'cuda:0'


def _build(workload, batch, graphed):
  import bench
  from rigl_amd import sparse_optimizers as SO, train, variables as V
  g = V.Graph(DEV)
  wl = bench.build_workload(workload, g, torch.device(DEV), batch, 0, None)
  inner = train.MomentumOptimizer(wl['lr'](batch), 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, grow_init='zeros', initial_acc_scale=0.0, **wl['opt'])
  gs = g.get_or_create_global_step()
  if graphed:
    step = train.GraphedStep(wl['loss'], opt, gs)
  else:
    def step():
      loss = wl['loss']()
      opt.minimize(loss, gs)
      return loss
  return dict(g=g, opt=opt, gs=gs, step=step, wl=wl)


def _stats(ms, nbytes):
  ms = sorted(ms)
  med = ms[len(ms) // 2]
  return {'bytes': nbytes, 'us_median': round(med * 1e3, 1), 'us_min': round(ms[0] * 1e3, 1), 'us_max': round(ms[-1] * 1e3, 1),
          'TBps_median': round(nbytes / med / 1e9, 3), 'TBps_best': round(nbytes / ms[0] / 1e9, 3)}


def bench_kernel(args):
  from rigl_amd import checkpoint, ops
  r = _build('resnet50', 8, False)
  state = checkpoint.TrainingState(r['g'], r['opt'])
  sizes, names = list(state._sizes), state.region_names()
  packed = state._packed_bytes
  del r, state
  sets = []
  for _ in range(args.ring):
    tensors = [torch.randint(0, 255, (s,), dtype=torch.uint8, device=DEV) for s in sizes]
    table = ops.state_table(tensors)
    sets.append(dict(tensors=tensors, table=table, staging=torch.zeros(packed, dtype=torch.uint8, device=DEV),
                     flat=torch.randint(0, 255, (packed,), dtype=torch.uint8, device=DEV)))
  digests = torch.zeros(2 * len(sizes), dtype=torch.int64, device=DEV)
  ws = torch.zeros(max(ops.state_workspace_bytes(sets[0]['table']), 256), dtype=torch.uint8, device=DEV)
  turn = [0]

  def timed(fn):
    ms = []
    for i in range(args.reps + 5):
      s = sets[turn[0] % len(sets)]
      turn[0] += 1
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn(s)
      e1.record()
      e1.synchronize()
      if i >= 5:
        ms.append(e0.elapsed_time(e1))
    return ms
  arms = [('copy', lambda s: s['staging'].copy_(s['flat'])),
          ('gather', lambda s: ops.state_gather(s['table'], s['staging'], digests, workspace_buffer=ws)),
          ('scatter', lambda s: ops.state_scatter(s['table'], s['staging'], digests, workspace_buffer=ws)),
          ('copy_again', lambda s: s['staging'].copy_(s['flat']))]
  out = {'what': 'kernel', 'regions': len(sizes), 'state_bytes': sum(sizes), 'packed_bytes': packed, 'reps': args.reps,
         'ring_sets': args.ring, 'largest': sorted(zip(sizes, names))[-3:]}
  for name, fn in arms:
    out[name] = _stats(timed(fn), 2 * packed)                    # every byte is read once and written once
  print(json.dumps(out), flush=True)
  return out


def bench_snapshot(args):
  from rigl_amd import checkpoint
  r = _build('resnet50', 8, False)
  state = checkpoint.TrainingState(r['g'], r['opt'])
  out = {'what': 'snapshot', 'packed_bytes': state._packed_bytes, 'regions': len(state.region_names()), 'reps': 8}
  state.snapshot().release()                                     # buffers are made
  torch.cuda.synchronize()
  for arm in ('released', 'kept'):
    call, copy_out, kept = [], [], None
    for _ in range(out['reps'] + 1):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      snap = state.snapshot()
      t1 = time.perf_counter()
      snap.wait()
      t2 = time.perf_counter()
      call.append((t1 - t0) * 1e3)
      copy_out.append((t2 - t1) * 1e3)
      if arm == 'released':
        snap.release()
      else:
        kept = snap                                              # alive and unsaved: the next snapshot() moves it out first
    call, copy_out = sorted(call[1:]), sorted(copy_out[1:])
    out[arm] = {'call_ms_median': round(call[len(call) // 2], 3), 'call_ms_min': round(call[0], 3), 'call_ms_max': round(call[-1], 3),
                'copy_out_ms_median': round(copy_out[len(copy_out) // 2], 3)}
  del kept
  print(json.dumps(out), flush=True)
  return out


def trace_csv(db, out_dir):
  import sqlite3
  cur = sqlite3.connect(db).cursor()
  groups = {}
  for name, gx, wx, dur in cur.execute('select name, grid_x, workgroup_x, duration from kernels'):
    if 'kstate' in name or 'copyBuffer' in name:
      short = name.split('(')[0].replace('void ', '').replace('rigl::kstate::', '')
      groups.setdefault((short, gx // wx), []).append(dur / 1e3)
  os.makedirs(out_dir, exist_ok=True)
  with open(os.path.join(out_dir, 'kernel_trace.csv'), 'w') as fh:
    fh.write('kernel,workgroups,calls,median_us,min_us,max_us\n')
    for (name, grid), v in sorted(groups.items()):
      v.sort()
      fh.write('%s,%d,%d,%.1f,%.1f,%.1f\n' % (name, grid, len(v), v[len(v) // 2], v[0], v[-1]))


def bench_wrn22(args):
  from rigl_amd import checkpoint, tf_checkpoint
  where = args.dir or tempfile.mkdtemp(prefix='ckpt_bench_')
  os.makedirs(where, exist_ok=True)
  arms = {a: _build('wrn22', 128, True) for a in ('none', 'snapshot', 'tf_bundle')}
  st = arms['snapshot']
  st['state'] = checkpoint.TrainingState(st['g'], st['opt'], model=st['wl'].get('model'))
  for r in arms.values():
    for _ in range(12):
      r['step']()
  torch.cuda.synchronize()
  stalls, sizes, writer = [], {}, [None]

  def checkpoint_now(name, r, i):
    if name == 'snapshot':
      if writer[0] is not None:
        writer[0].join()                                         # a single writer: files land in order, one at a time
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      snap = r['state'].snapshot()
      e1.record()
      stalls.append((e0, e1))
      path = os.path.join(where, 'state.ckpt')
      writer[0] = threading.Thread(target=snap.save, args=(path,))
      writer[0].start()
    elif name == 'tf_bundle':
      tf_checkpoint.save_graph(os.path.join(where, 'bundle'), r['g'])

  secs = {a: [] for a in arms}
  for _ in range(args.rounds):
    for name, r in arms.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for i in range(args.block):
        r['step']()
        if (i + 1) % args.every == 0:
          checkpoint_now(name, r, i)
      torch.cuda.synchronize()
      if name == 'snapshot' and writer[0] is not None:
        writer[0].join()                                         # the block is over when its last file is on disk
        writer[0] = None
      secs[name].append((time.perf_counter() - t0) / args.block)
  sizes['state.ckpt'] = os.path.getsize(os.path.join(where, 'state.ckpt'))
  sizes['tf_bundle'] = sum(os.path.getsize(os.path.join(where, f)) for f in os.listdir(where) if f.startswith('bundle'))
  stall_ms = sorted(a.elapsed_time(b) for a, b in stalls)
  out = {'what': 'wrn22', 'batch': 128, 'block': args.block, 'every': args.every, 'rounds': args.rounds, 'file_bytes': sizes,
         'stall_us_median': round(stall_ms[len(stall_ms) // 2] * 1e3, 1), 'stall_us_min': round(stall_ms[0] * 1e3, 1),
         'stall_us_max': round(stall_ms[-1] * 1e3, 1), 'snapshots': len(stall_ms), 'regions': len(st['state'].region_names())}
  for name, r in arms.items():
    v = sorted(secs[name])
    med = v[len(v) // 2]
    out[name] = {'images_per_s_median': round(128 / med, 1), 'images_per_s_min': round(128 / v[-1], 1),
                 'images_per_s_max': round(128 / v[0], 1), 'ms_per_step_median': round(med * 1e3, 4),
                 'replays': r['step'].replays, 'eager_steps': r['step'].eager_steps, 'graphs': len(r['step']._graphs)}
  if not args.dir:
    shutil.rmtree(where, ignore_errors=True)
  print(json.dumps(out), flush=True)
  return out


def tables(rows):
  L = []
  for r in rows:
    if r['what'] == 'kernel':
      L += ['| | bytes read + written | median | min - max | median rate | best rate |', '|---|---|---|---|---|---|']
      for name in ('copy', 'gather', 'scatter', 'copy_again'):
        a = r[name]
        L.append('| %s | %d | %.1f us | %.1f - %.1f us | %.3f TB/s | %.3f TB/s |' % (
            name, a['bytes'], a['us_median'], a['us_min'], a['us_max'], a['TBps_median'], a['TBps_best']))
      L.append('')
    if r['what'] == 'snapshot':
      L += ['| snapshot before | snapshot() host time median (min - max) | copy-out then lands after |', '|---|---|---|']
      for name in ('released', 'kept'):
        a = r[name]
        L.append('| %s | %.3f ms (%.3f - %.3f) | %.3f ms |' % (name, a['call_ms_median'], a['call_ms_min'], a['call_ms_max'], a['copy_out_ms_median']))
      L.append('')
    if r['what'] == 'wrn22':
      L += ['| arm | images/s median (min - max) | ms per step | over none |', '|---|---|---|---|']
      for name in ('none', 'snapshot', 'tf_bundle'):
        a = r[name]
        L.append('| %s | %s (%s - %s) | %.4f | %.4f |' % (name, a['images_per_s_median'], a['images_per_s_min'], a['images_per_s_max'],
                                                         a['ms_per_step_median'], a['images_per_s_median'] / r['none']['images_per_s_median']))
      L.append('')
  return '\n'.join(L)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=40)
  ap.add_argument('--ring', type=int, default=3)
  ap.add_argument('--block', type=int, default=200)
  ap.add_argument('--every', type=int, default=50)
  ap.add_argument('--skip', default='')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'checkpoint'))
  ap.add_argument('--dir', default=None)
  ap.add_argument('--trace', default=None)
  args = ap.parse_args()
  if args.trace:
    return trace_csv(args.trace, args.out)
  if not torch.cuda.is_available():
    raise SystemExit('checkpoint_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  box = {'what': 'box', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'lib_sha16': sha}
  print(json.dumps(box), flush=True)
  skip = set(args.skip.split(','))
  rows = [box]
  if 'kernel' not in skip:
    rows.append(bench_kernel(args))
  if 'snapshot' not in skip:
    rows.append(bench_snapshot(args))
  if 'wrn22' not in skip:
    rows.append(bench_wrn22(args))
  os.makedirs(args.out, exist_ok=True)
  with open(os.path.join(args.out, 'checkpoint_bench.jsonl'), 'w') as fh:
    for r in rows:
      fh.write(json.dumps(r) + '\n')
  with open(os.path.join(args.out, 'tables.md'), 'w') as fh:
    fh.write(tables(rows))


if __name__ == '__main__':
  main()
