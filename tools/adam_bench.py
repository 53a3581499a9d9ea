"""K3-Adam vs K3-momentum on a ResNet-50-sized arena (25.6 M fp32 parameters, 80 % of the mask bits off), timed
alternately in one process so both see the same clocks.  Prints one JSON line: ms per step and GB/s at the ALGORITHMIC
bytes of each update (what must cross HBM at least once):

  Adam:      w, m, v read + written, g read, 1 mask bit   = 28.125 B / parameter  (+ 2 B with the bf16 shadow)
  momentum:  w, a read + written, g read, 1 mask bit      = 20.125 B / parameter  (bench.py's figure, no shadow)

  python tools/adam_bench.py [--n 25600000] [--iters 50] [--reps 5] [--shadow]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rigl_amd import ops  # noqa: E402

PEAK_GBS = 8000.0


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=25_600_000)
  ap.add_argument('--iters', type=int, default=50, help='launches per timed block')
  ap.add_argument('--reps', type=int, default=5, help='alternating blocks per kernel (the median is reported)')
  ap.add_argument('--shadow', action='store_true', help='Adam also writes the bf16 shadow (counted as 2 B)')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  n = (args.n + 63) // 64 * 64
  gen = torch.Generator(device=dev)
  gen.manual_seed(0)
  w = torch.randn(n, device=dev, generator=gen)
  g = torch.randn(n, device=dev, generator=gen) * 1e-3
  m = torch.zeros(n, device=dev)
  v = torch.zeros(n, device=dev)
  a = torch.zeros(n, device=dev)
  bits = ops.mask_pack((torch.rand(n, device=dev, generator=gen) < 0.2).float())
  bp = torch.tensor([0.9, 0.999], dtype=torch.float32, device=dev)
  shadow = torch.empty(n, dtype=torch.bfloat16, device=dev) if args.shadow else None

  def adam():
    ops.masked_adam(w, g, m, v, bp, 1e-4, mask_bits=bits, weight_decay=1e-4, w_shadow=shadow)

  def mom():
    ops.masked_sgd_momentum(w, g, 1e-4, momentum=a, mask_bits=bits, mu=0.9, weight_decay=1e-4, nesterov=True)

  def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters

  for fn in (adam, mom, adam, mom):       # warm-up (code objects, clocks)
    block(fn)
  t_adam, t_mom = [], []
  for _ in range(args.reps):
    t_adam.append(block(adam))
    t_mom.append(block(mom))
  med = lambda xs: sorted(xs)[len(xs) // 2]
  ms_a, ms_m = med(t_adam), med(t_mom)
  b_adam = 28.125 + (2.0 if args.shadow else 0.0)
  b_mom = 20.125
  gbs_a = n * b_adam / (ms_a * 1e-3) / 1e9
  gbs_m = n * b_mom / (ms_m * 1e-3) / 1e9
  print(json.dumps({'n': n, 'shadow': bool(args.shadow), 'iters': args.iters, 'reps': args.reps,
                    'adam_ms': round(ms_a, 4), 'adam_bytes_per_param': b_adam, 'adam_gbs': round(gbs_a, 1),
                    'adam_frac_of_8tbs': round(gbs_a / PEAK_GBS, 3),
                    'momentum_ms': round(ms_m, 4), 'momentum_bytes_per_param': b_mom, 'momentum_gbs': round(gbs_m, 1),
                    'momentum_frac_of_8tbs': round(gbs_m / PEAK_GBS, 3),
                    'adam_ms_all': [round(x, 4) for x in t_adam], 'momentum_ms_all': [round(x, 4) for x in t_mom]}))


if __name__ == '__main__':
  main()
