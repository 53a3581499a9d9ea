"""Two builds of librigl_hip.so -- a parent commit's and the working tree's -- timed on K3 in ONE process on the SAME
tensors, in alternating blocks (tools/adam_bench.py's setting: 25.6 M parameters, 80 % of the mask bits off, wd 1e-4), so
neither the clocks nor the placement of the tensors differ between the two.  Prints one JSON line: median / min / max ms
per launch of masked Adam and masked Nesterov momentum for each build, and every block.

  python tools/k3_ab.py <parent librigl_hip.so> <branch librigl_hip.so>
"""
import ctypes as C
import json
import sys

import torch

P, F, I64, I32 = C.c_void_p, C.c_float, C.c_int64, C.c_int32


def load(path):
  lib = C.CDLL(path, mode=C.RTLD_LOCAL)
  lib.rigl_masked_sgd_momentum.restype = C.c_int
  lib.rigl_masked_sgd_momentum.argtypes = [I64, P, P, P, P, F, F, F, F, I32, P, P]
  lib.rigl_masked_adam.restype = C.c_int
  lib.rigl_masked_adam.argtypes = [I64, P, P, P, P, P, P, F, F, F, F, F, F, P, P]
  lib.rigl_mask_pack.restype = C.c_int
  lib.rigl_mask_pack.argtypes = [P, P, I64, P]
  return lib


def main():
  dev = torch.device('cuda:0')
  libs = {'parent': load(sys.argv[1]), 'branch': load(sys.argv[2])}
  n = 25_600_000
  gen = torch.Generator(device=dev)
  gen.manual_seed(0)
  w = torch.randn(n, device=dev, generator=gen)
  g = torch.randn(n, device=dev, generator=gen) * 1e-3
  m, v, a = (torch.zeros(n, device=dev) for _ in range(3))
  mask = (torch.rand(n, device=dev, generator=gen) < 0.2).float()
  bits = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  assert libs['parent'].rigl_mask_pack(mask.data_ptr(), bits.data_ptr(), n, st) == 0
  bp = torch.tensor([0.9, 0.999], dtype=torch.float32, device=dev)
  p = lambda t: C.c_void_p(t.data_ptr())

  def adam(lib):
    assert lib.rigl_masked_adam(n, p(w), p(m), p(v), p(g), p(bits), p(bp), 1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0, None, st) == 0

  def mom(lib):
    assert lib.rigl_masked_sgd_momentum(n, p(w), p(a), p(g), p(bits), 1e-4, 0.9, 1e-4, 1.0, 1, None, st) == 0

  def block(fn, lib, iters=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
      fn(lib)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters

  for _ in range(2):
    for lib in libs.values():
      block(adam, lib)
      block(mom, lib)
  out = {k + '_' + b: [] for k in ('adam', 'momentum') for b in libs}
  for _ in range(20):
    for b, lib in libs.items():
      out['adam_' + b].append(round(block(adam, lib), 4))
    for b, lib in libs.items():
      out['momentum_' + b].append(round(block(mom, lib), 4))
  med = lambda xs: sorted(xs)[len(xs) // 2]
  print(json.dumps({'n': n, 'iters': 50, 'blocks': 20,
                    'median_ms': {k: med(x) for k, x in out.items()}, 'min_ms': {k: min(x) for k, x in out.items()},
                    'max_ms': {k: max(x) for k, x in out.items()}, 'all_ms': out}))


if __name__ == '__main__':
  main()
