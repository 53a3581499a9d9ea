"""rigl_magnitude_prune_batched (gradual magnitude pruning's mask update) vs rigl_topk_mask_batched (DNW's per-step
top-k) over the same masked tensor sets -- ResNet-50's 54 (25.5 M weights) and WRN-22's -- timed with device events
after warm-up, the two calls alternating in one process.  Prints one JSON line per set.

Bytes are those of the passes each call makes over its per-weight data (per-layer state is ignored):
  magnitude prune: three radix-digit passes read W (4 B each; the first also reads the old bitmap, 1/8 B),
                   the apply pass reads W and writes the bitmap (4 + 1/8 B)          = 16.25 B / weight
  top-k (DNW):     three digit passes read the score (4 B; the first also reads the bitmap, 1/8 B), the tie count
                   reads nothing when the k-th score is unique, the apply pass reads the score and writes the
                   bitmap (4 + 1/8 B)                                                = 16.25 B / weight
                   (plus the |W| score buffer DNW forms before the call, not timed here)

  python tools/prune_bench.py [--iters 20] [--reps 7] [--sparsity 0.8]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigl_amd import ops  # noqa: E402
from tests.golden import layer_shapes  # noqa: E402

PEAK_GBS = 8000.0
BYTES_PER_WEIGHT = {'magnitude_prune': 16.25, 'topk_mask': 16.25}


def _k(n, s):
  return max(1, int(np.rint(np.float32(np.float32(n) * (np.float32(1) - np.float32(s))))))


def bench_set(name, shapes, args, dev):
  gen = torch.Generator(device=dev)
  gen.manual_seed(0)
  ns = [int(np.prod(sh)) for sh in shapes]
  w = [torch.randn(n, device=dev, generator=gen) for n in ns]
  score = [x.abs() for x in w]
  bits_a = [torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev) for n in ns]
  bits_b = [torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev) for n in ns]
  thr = torch.zeros(len(ns), dtype=torch.float32, device=dev)
  mag_items = [(w[i], bits_a[i], thr[i:i + 1], _k(n, args.sparsity)) for i, n in enumerate(ns)]
  topk_items = [(score[i], _k(n, args.sparsity), bits_b[i]) for i, n in enumerate(ns)]

  def mag():
    ops.magnitude_prune_batched(mag_items, 0.0)

  def topk():
    ops.topk_mask_batched(topk_items)

  def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters

  for fn in (mag, topk, mag, topk):      # warm-up: code objects, workspaces, clocks
    block(fn)
  t_mag, t_topk = [], []
  for _ in range(args.reps):
    t_mag.append(block(mag))
    t_topk.append(block(topk))
  # both select the same k largest |W|: with distinct values the bitmaps agree
  same = all(torch.equal(a, b) for a, b in zip(bits_a, bits_b))
  ops.prof_collect()
  ops.prof_enable(True)
  mag()
  ops.prof_enable(False)
  prof_ms, prof_n = ops.prof_collect()['magnitude_prune']
  med = lambda xs: sorted(xs)[len(xs) // 2]
  n_tot = sum(ns)
  out = {'set': name, 'layers': len(ns), 'weights': n_tot, 'sparsity': args.sparsity, 'iters': args.iters,
         'reps': args.reps, 'bitmaps_identical': bool(same), 'profiler_magnitude_prune_ms': round(prof_ms, 4),
         'profiler_magnitude_prune_calls': int(prof_n)}
  for key, ts in (('magnitude_prune', t_mag), ('topk_mask', t_topk)):
    ms = med(ts)
    gbs = n_tot * BYTES_PER_WEIGHT[key] / (ms * 1e-3) / 1e9
    out.update({key + '_ms': round(ms, 4), key + '_gbs': round(gbs, 1), key + '_frac_of_8tbs': round(gbs / PEAK_GBS, 3),
                key + '_ms_all': [round(x, 4) for x in ts]})
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20, help='calls per timed block')
  ap.add_argument('--reps', type=int, default=7, help='alternating blocks per call (the median is reported)')
  ap.add_argument('--sparsity', type=float, default=0.8)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('prune_bench: needs a GPU')
  dev = torch.device('cuda:0')
  for name, shapes in (('resnet50', list(layer_shapes.resnet50().values())),
                       ('wrn22', list(layer_shapes.wide_resnet().values()))):
    print(json.dumps(bench_set(name, shapes, args, dev)), flush=True)


if __name__ == '__main__':
  main()
