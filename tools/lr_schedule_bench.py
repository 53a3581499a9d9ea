"""What a per-step learning-rate schedule costs under graph replay (profiles/lrsched/README.md).  WRN-22 at batch 128 under
train.GraphedStep, four optimizers side by side in one process, JSON-printed:

  (1) const        learning_rate = 0.1: the control (bench.py --graph's configuration)
  (2) warmup_dev   the MobileNet-style ImageNet schedule, inside its linear warm-up for the whole run, as a
                   schedules.Schedule: the rate is computed and read on the device, one graph is replayed
  (3) warmup_host  the same schedule as host_only(): a callable whose value changes every step, so GraphedStep captures
                   nothing and every step runs eagerly (what a per-step schedule got before the device path)
  (4) sgdr_dev     cosine_decay_restarts (--use_sgdr) on the device path

  step      the four arms timed in alternating blocks of --block steps (host clock around a device synchronise), median
            images/s over --rounds
  launches  kernel nodes of the captured step of (1) and (2) (hipGraphGetNodes on the graph GraphedStep captured)

Usage: python tools/lr_schedule_bench.py [--rounds 7] [--block 100] [--skip-step] [--skip-launches]
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
ARMS = ('const', 'warmup_dev', 'warmup_host', 'sgdr_dev')


def learning_rate(arm, batch):
  from rigl_amd import schedules
  if arm == 'const':
    return 0.1
  if arm == 'sgdr_dev':
    return schedules.imagenet_lr_schedule(0.2, batch, use_sgdr=True, train_steps=10 ** 6)
  # 8 epochs of 1281167 / batch steps: the run never leaves the warm-up
  sched = schedules.imagenet_lr_schedule(0.2, batch, model_architecture='mobilenet_v1')
  return sched if arm == 'warmup_dev' else sched.host_only()


def build(arm, batch):
  """The wrn22 configuration of bench.py (ERK 0.8, RigL dT=100 drop 0.3 constant, Nesterov 0.9) on a graph of its own."""
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.Graph(DEV)
  model = wide_resnet.WideResNet(g, depth=22, width=1)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  images, labels = wide_resnet.synthetic_batch(batch, DEV)
  inner = train.MomentumOptimizer(learning_rate(arm, batch), 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 75000, 100, drop_fraction=0.3, drop_fraction_anneal='constant')
  gs = g.get_or_create_global_step()
  loss_fn = lambda: model.loss(images, labels)
  return dict(model=model, inner=inner, opt=opt, gs=gs, loss_fn=loss_fn, step=train.GraphedStep(loss_fn, opt, gs),
              train=train)


def bench_step(args):
  runs = {a: build(a, args.batch) for a in ARMS}
  for a in ARMS:                                     # warm-up: eager steps, capture, first replays
    for _ in range(args.warmup):
      runs[a]['step']()
  torch.cuda.synchronize()
  rates = {a: [] for a in ARMS}
  for _ in range(args.rounds):
    for a in ARMS:
      st = runs[a]['step']
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.block):
        st()
      torch.cuda.synchronize()
      rates[a].append(args.batch * args.block / (time.perf_counter() - t0))
  out = {'what': 'step', 'workload': 'wrn22', 'batch': args.batch, 'block_steps': args.block, 'rounds': args.rounds}
  for a in ARMS:
    v = sorted(rates[a])
    st = runs[a]['step']
    out[a] = {'images_per_s_median': round(v[len(v) // 2], 1), 'min': round(v[0], 1), 'max': round(v[-1], 1),
              'replays': st.replays, 'eager_steps': st.eager_steps, 'graphs': len(st._graphs),   # pylint: disable=protected-access
              'global_step': int(runs[a]['gs'].value)}
    inner = runs[a]['inner']
    if inner.lr_on_device():
      out[a]['device_counter'] = int(inner.device_lr.counter.tensor.cpu()[0])
      out[a]['device_lr'] = float(inner.device_lr.rate.cpu()[0])
  med = lambda a: out[a]['images_per_s_median']
  out['warmup_dev_over_const'] = round(med('warmup_dev') / med('const'), 4)
  out['sgdr_dev_over_const'] = round(med('sgdr_dev') / med('const'), 4)
  out['warmup_dev_over_warmup_host'] = round(med('warmup_dev') / med('warmup_host'), 4)
  out['sgdr_dev_over_warmup_host'] = round(med('sgdr_dev') / med('warmup_host'), 4)
  print(json.dumps(out), flush=True)
  return runs


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
  """A fresh GraphedStep per arm whose graph keeps its hipGraph_t, stepped until it has captured."""
  out = {'what': 'launches', 'workload': 'wrn22', 'batch': args.batch}
  plain = torch.cuda.CUDAGraph
  torch.cuda.CUDAGraph = lambda *a, **k: plain(*a, keep_graph=True, **k)
  try:
    for a in ('const', 'warmup_dev'):
      run = runs[a] if runs else build(a, args.batch)
      st = run['train'].GraphedStep(run['loss_fn'], run['opt'], run['gs'])
      for _ in range(12):
        st()
        if st.replays:
          break
      torch.cuda.synchronize()
      (graph, _), = st._graphs.values()             # pylint: disable=protected-access
      kernels, nodes = _kernel_nodes(graph)
      out[a] = {'kernel_nodes': kernels, 'graph_nodes': nodes}
  finally:
    torch.cuda.CUDAGraph = plain
  out['added_by_schedule'] = out['warmup_dev']['kernel_nodes'] - out['const']['kernel_nodes']
  out['expected_added'] = 1                          # the rigl_lr_schedule_step launch
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--block', type=int, default=100)
  ap.add_argument('--warmup', type=int, default=30)
  ap.add_argument('--skip-step', action='store_true')
  ap.add_argument('--skip-launches', action='store_true')
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('lr_schedule_bench: no GPU visible; nothing is measured without one')
  from rigl_amd import _lib
  with open(_lib.LIB_PATH, 'rb') as fh:
    sha = hashlib.sha256(fh.read()).hexdigest()[:16]
  print(json.dumps({'what': 'box', 'host': socket.gethostname(), 'device': torch.cuda.get_device_name(0),
                    'torch': torch.__version__, 'lib_sha16': sha}), flush=True)
  runs = None
  if not args.skip_step:
    runs = bench_step(args)
  if not args.skip_launches:
    count_launches(args, runs)


if __name__ == '__main__':
  main()
