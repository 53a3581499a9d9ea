"""What dropout costs (profiles/dropout/README.md).  Three measurements in one process, each JSON-printed:

  (a) step    WRN-22 at batch 128 under train.GraphedStep with droprate 0 and 0.3: two models side by side, timed in
              alternating blocks of --block steps (host clock around a device synchronise), median images/s over --rounds.
  (b) kernel  rigl_dropout_fwd / rigl_dropout_bwd on a 256 MB bf16 tensor next to y.copy_(x) on the same tensor, alternating,
              device events, median over --reps.  Bytes: fwd and bwd move 2 * 256 MB + 16 MB of bits, the copy 2 * 256 MB.
  (c) launches  kernel nodes of the captured step of each model (hipGraphGetNodes on the graph GraphedStep captured).

Usage: python tools/dropout_bench.py [--rounds 7] [--block 100] [--reps 20] [--skip-step] [--skip-kernel] [--skip-launches]
"""
import argparse
import ctypes
import hashlib
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'
RATES = (0.0, 0.3)


def build(rate, batch):
  """The wrn22 configuration of bench.py (ERK 0.8, RigL dT=100 drop 0.3 constant, Nesterov 0.9, lr 0.1) on a graph of its own."""
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.Graph(DEV)
  model = wide_resnet.WideResNet(g, depth=22, width=1, droprate=rate)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  images, labels = wide_resnet.synthetic_batch(batch, DEV)
  inner = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 75000, 100, drop_fraction=0.3, drop_fraction_anneal='constant')   # (its graph: inner's)
  gs = g.get_or_create_global_step()
  loss_fn = lambda: model.loss(images, labels)
  return dict(model=model, opt=opt, gs=gs, loss_fn=loss_fn, step=train.GraphedStep(loss_fn, opt, gs), train=train)


def bench_step(args):
  runs = {r: build(r, args.batch) for r in RATES}
  for r in RATES:                                    # warm-up: eager steps, capture, first replays
    for _ in range(args.warmup):
      runs[r]['step']()
  torch.cuda.synchronize()
  rates = {r: [] for r in RATES}
  for _ in range(args.rounds):
    for r in RATES:
      st = runs[r]['step']
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.block):
        st()
      torch.cuda.synchronize()
      rates[r].append(args.batch * args.block / (time.perf_counter() - t0))
  out = {'what': 'step', 'workload': 'wrn22', 'batch': args.batch, 'block_steps': args.block, 'rounds': args.rounds}
  for r in RATES:
    v = sorted(rates[r])
    out['droprate_%g' % r] = {'images_per_s_median': round(v[len(v) // 2], 1), 'min': round(v[0], 1), 'max': round(v[-1], 1),
                              'replays': runs[r]['step'].replays, 'eager_steps': runs[r]['step'].eager_steps}
  out['ratio_0.3_over_0'] = round(out['droprate_0.3']['images_per_s_median'] / out['droprate_0']['images_per_s_median'], 4)
  out['dropout_step_counter'] = int(runs[0.3]['model'].dropout_state.step)
  print(json.dumps(out), flush=True)
  return runs


def bench_kernel(args):
  from rigl_amd import ops
  n = args.mb * (1 << 20) // 2
  x = torch.randn(n, device=DEV).to(torch.bfloat16)
  y = torch.empty_like(x)
  bits = torch.empty(n // 8, dtype=torch.uint8, device=DEV)
  step = torch.zeros(1, dtype=torch.int32, device=DEV)
  fns = {'copy': lambda: y.copy_(x),
         'fwd': lambda: ops.dropout_fwd(x, 0.3, 12345, step, y=y, bits=bits),
         'bwd': lambda: ops.dropout_bwd(x, bits, 0.3, dx=y)}
  nbytes = {'copy': 4 * n, 'fwd': 4 * n + n // 8, 'bwd': 4 * n + n // 8}
  for _ in range(3):
    for f in fns.values():
      f()
  torch.cuda.synchronize()
  ms = {k: [] for k in fns}
  for _ in range(args.reps):
    for k, f in fns.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      f()
      b.record()
      b.synchronize()
      ms[k].append(a.elapsed_time(b))
  out = {'what': 'kernel', 'dtype': 'bf16', 'tensor_mb': args.mb, 'reps': args.reps}
  for k in fns:
    v = sorted(ms[k])
    med = v[len(v) // 2]
    out[k] = {'median_ms': round(med, 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4), 'bytes': nbytes[k],
              'gb_per_s': round(nbytes[k] / med / 1e6, 1)}
  for k in ('fwd', 'bwd'):
    out['%s_over_copy' % k] = round(out[k]['gb_per_s'] / out['copy']['gb_per_s'], 3)
  print(json.dumps(out), flush=True)


def _kernel_nodes(graph):
  """Kernel nodes of a captured torch.cuda.CUDAGraph(keep_graph=True)."""
  with open('/proc/self/maps') as fh:               # the HIP runtime this process already runs on, not a second copy
    paths = sorted({line.split()[-1] for line in fh if 'libamdhip64' in line})
  if len(paths) != 1:
    raise RuntimeError('expected one loaded libamdhip64, found %r' % (paths,))
  hip = ctypes.CDLL(paths[0])
  raw = ctypes.c_void_p(graph.raw_cuda_graph())
  n = ctypes.c_size_t(0)
  if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
    raise RuntimeError('hipGraphGetNodes failed')
  nodes = (ctypes.c_void_p * n.value)()
  if hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
    raise RuntimeError('hipGraphGetNodes failed')
  kernels = 0
  for node in nodes:
    t = ctypes.c_int(-1)
    if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t)) != 0:
      raise RuntimeError('hipGraphNodeGetType failed')
    kernels += t.value == 0                          # hipGraphNodeTypeKernel
  return kernels, n.value


def count_launches(args, runs):
  """A fresh GraphedStep per model whose graph keeps its hipGraph_t, stepped until it has captured."""
  out = {'what': 'launches', 'workload': 'wrn22', 'batch': args.batch}
  plain = torch.cuda.CUDAGraph
  torch.cuda.CUDAGraph = lambda *a, **k: plain(*a, keep_graph=True, **k)
  try:
    for r in RATES:
      run = runs[r] if runs else build(r, args.batch)
      st = run['train'].GraphedStep(run['loss_fn'], run['opt'], run['gs'])
      for _ in range(12):
        st()
        if st.replays:
          break
      torch.cuda.synchronize()
      (graph, _), = st._graphs.values()             # pylint: disable=protected-access
      kernels, nodes = _kernel_nodes(graph)
      out['droprate_%g' % r] = {'kernel_nodes': kernels, 'graph_nodes': nodes, 'blocks': len(run['model'].blocks)}
  finally:
    torch.cuda.CUDAGraph = plain
  out['added_by_dropout'] = out['droprate_0.3']['kernel_nodes'] - out['droprate_0']['kernel_nodes']
  out['expected_added'] = 1 + 2 * out['droprate_0.3']['blocks']       # one advance + a forward and a backward per block
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--block', type=int, default=100)
  ap.add_argument('--warmup', type=int, default=30)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--mb', type=int, default=256)
  ap.add_argument('--skip-step', action='store_true')
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-launches', action='store_true')
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('dropout_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  print(json.dumps({'what': 'box', 'host': socket.gethostname(), 'device': torch.cuda.get_device_name(0),
                    'torch': torch.__version__, 'lib_sha16': sha}), flush=True)
  runs = None
  if not args.skip_kernel:
    bench_kernel(args)
  if not args.skip_step:
    runs = bench_step(args)
  if not args.skip_launches:
    count_launches(args, runs)


if __name__ == '__main__':
  main()
