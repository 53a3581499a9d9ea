"""What the device CIFAR input pipeline costs (profiles/input/README.md).  Measurements in one process, each JSON-printed:

  (a) kernel  rigl_cifar_batch + rigl_cifar_advance at batch 128 and 1024, bf16 and fp32, on a 50 000-image dataset of random
              bytes, next to a device-to-device copy of the same output bytes.  The launches are a few microseconds long, so
              --chain of them are captured into one graph and the graph is replayed between two device events: per-iteration
              time = replay time / chain, median over --reps replays, loader and copy alternating.
  (b) step    WRN-22 at batch 128 under train.GraphedStep (the wrn22 configuration of bench.py): the parent's fixed synthetic
              batch, the same a second time (the spread of two identical configurations), and DeviceCifar.next_batch() inside
              loss_fn -- three models side by side, alternating blocks of --block steps, host clock around a device
              synchronise, median images/s over --rounds.
  (c) launches  kernel nodes of the captured step with and without the loader.
  (d) host    the NumPy reference of the pipeline (tests/input_ref.py) and a vectorised NumPy pipeline (what a user would
              write: same standardization, pad, crop, flip; np.random draws and permutation), each plus one host-to-device copy
              per batch, in images/s on this host.

Usage: python tools/input_bench.py [--rounds 7] [--block 100] [--reps 20] [--chain 100] [--skip-kernel] [--skip-step]
                                   [--skip-launches] [--skip-host]
"""
import argparse
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
N_IMAGES = 50000


def device_dataset(n=N_IMAGES, seed=0):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  images = torch.randint(0, 256, (n, 32, 32, 3), generator=gen, device=DEV, dtype=torch.uint8)
  labels = torch.randint(0, 10, (n,), generator=gen, device=DEV, dtype=torch.int32)
  return images, labels


def _median_spread(v):
  v = sorted(v)
  return v[len(v) // 2], v[0], v[-1]


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def _chained_graph(fn, chain):
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(3):
      fn()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    for _ in range(chain):
      fn()
  return graph


def bench_kernel(args):
  from rigl_amd import data
  images, labels = device_dataset()
  for batch in (128, 1024):
    for dtype in (torch.bfloat16, torch.float32):
      dc = data.DeviceCifar(images, labels, batch, seed=1234, dtype=dtype, device=DEV)
      src, dst = torch.randn(batch, 32, 32, 3, device=DEV).to(dtype), torch.empty(batch, 32, 32, 3, dtype=dtype, device=DEV)
      graphs = {'loader': _chained_graph(dc.next_batch, args.chain), 'copy': _chained_graph(lambda: dst.copy_(src), args.chain)}
      for g in graphs.values():
        g.replay()
      torch.cuda.synchronize()
      us = {k: [] for k in graphs}
      for _ in range(args.reps):
        for k, g in graphs.items():
          a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          a.record()
          g.replay()
          b.record()
          b.synchronize()
          us[k].append(a.elapsed_time(b) * 1e3 / args.chain)
      out_bytes = dst.numel() * dst.element_size()
      out = {'what': 'kernel', 'batch': batch, 'dtype': str(dtype).replace('torch.', ''), 'chain': args.chain, 'reps': args.reps,
             'dataset_images': N_IMAGES, 'output_bytes': out_bytes, 'read_bytes': batch * 3072,
             'loader_launches_per_iteration': 3, 'counter_after': dc.position()}
      for k in graphs:
        med, lo, hi = _median_spread(us[k])
        out[k] = {'median_us': round(med, 3), 'min_us': round(lo, 3), 'max_us': round(hi, 3)}
      out['loader_over_copy'] = round(out['loader']['median_us'] / out['copy']['median_us'], 3)
      print(json.dumps(out), flush=True)


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------
def build(feed, batch):
  """The wrn22 configuration of bench.py (ERK 0.8, RigL dT=100 drop 0.3 constant, Nesterov 0.9, lr 0.1) on a graph of its own;
  ``feed``: 'fixed' = the parent's one synthetic batch, 'loader' = a DeviceCifar over 50 000 random-byte images."""
  from rigl_amd import data, sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.Graph(DEV)
  model = wide_resnet.WideResNet(g, depth=22, width=1)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  inner = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 75000, 100, drop_fraction=0.3, drop_fraction_anneal='constant')
  gs = g.get_or_create_global_step()
  dc = None
  if feed == 'loader':
    dc = data.DeviceCifar(*device_dataset(), batch, seed=1234, device=DEV)
    loss_fn = lambda: model.loss(*dc.next_batch())
  else:
    images, labels = wide_resnet.synthetic_batch(batch, DEV)
    loss_fn = lambda: model.loss(images, labels)
  return dict(model=model, opt=opt, gs=gs, loss_fn=loss_fn, step=train.GraphedStep(loss_fn, opt, gs), train=train, loader=dc)


FEEDS = ('fixed', 'loader', 'fixed_again')


def bench_step(args):
  runs = {f: build('loader' if f == 'loader' else 'fixed', args.batch) for f in FEEDS}
  for f in FEEDS:
    for _ in range(args.warmup):
      runs[f]['step']()
  torch.cuda.synchronize()
  rates = {f: [] for f in FEEDS}
  for _ in range(args.rounds):
    for f in FEEDS:
      st = runs[f]['step']
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.block):
        st()
      torch.cuda.synchronize()
      rates[f].append(args.batch * args.block / (time.perf_counter() - t0))
  out = {'what': 'step', 'workload': 'wrn22', 'batch': args.batch, 'block_steps': args.block, 'rounds': args.rounds}
  for f in FEEDS:
    med, lo, hi = _median_spread(rates[f])
    out[f] = {'images_per_s_median': round(med, 1), 'min': round(lo, 1), 'max': round(hi, 1), 'ms_per_step': round(1e3 * args.batch / med, 4),
              'replays': runs[f]['step'].replays, 'eager_steps': runs[f]['step'].eager_steps}
  out['loader_us_per_step_over_fixed'] = round(1e3 * (out['loader']['ms_per_step'] - out['fixed']['ms_per_step']), 2)
  out['fixed_again_us_per_step_over_fixed'] = round(1e3 * (out['fixed_again']['ms_per_step'] - out['fixed']['ms_per_step']), 2)
  out['loader_counter'] = runs['loader']['loader'].position()
  out['loader_steps_per_epoch'] = runs['loader']['loader'].steps_per_epoch
  print(json.dumps(out), flush=True)
  return runs


def count_launches(args, runs):
  import importlib.util
  spec = importlib.util.spec_from_file_location('dropout_bench', os.path.join(ROOT, 'tools', 'dropout_bench.py'))
  dropout_bench = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(dropout_bench)                # (its hipGraphGetNodes reader)
  _kernel_nodes = dropout_bench._kernel_nodes           # pylint: disable=protected-access
  out = {'what': 'launches', 'workload': 'wrn22', 'batch': args.batch}
  plain = torch.cuda.CUDAGraph
  torch.cuda.CUDAGraph = lambda *a, **k: plain(*a, keep_graph=True, **k)
  try:
    for f in ('fixed', 'loader'):
      run = runs[f] if runs else build(f, args.batch)
      st = run['train'].GraphedStep(run['loss_fn'], run['opt'], run['gs'])
      for _ in range(12):
        st()
        if st.replays:
          break
      torch.cuda.synchronize()
      (graph, _), = st._graphs.values()             # pylint: disable=protected-access
      kernels, nodes = _kernel_nodes(graph)
      out[f] = {'kernel_nodes': kernels, 'graph_nodes': nodes}
  finally:
    torch.cuda.CUDAGraph = plain
  out['added_by_loader'] = out['loader']['kernel_nodes'] - out['fixed']['kernel_nodes']
  print(json.dumps(out), flush=True)


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def _host_batch(images, idx, rng):
  """A vectorised NumPy statement of the pipeline for one batch: fp32 standardization, mirror pad, crop, flip."""
  x = images[idx].astype(np.float32)
  flat = x.reshape(len(idx), -1)
  mean = flat.mean(axis=1)
  std = np.maximum(flat.std(axis=1), np.float32(1.0 / np.sqrt(3072.0)))
  x = (x - mean[:, None, None, None]) / std[:, None, None, None]
  x = np.pad(x, ((0, 0), (4, 4), (4, 4), (0, 0)), mode='symmetric')
  oy, ox, flip = rng.randint(0, 9, len(idx)), rng.randint(0, 9, len(idx)), rng.uniform(size=len(idx)) < 0.5
  out = np.empty((len(idx), 32, 32, 3), dtype=np.float32)
  for i in range(len(idx)):
    crop = x[i, oy[i]:oy[i] + 32, ox[i]:ox[i] + 32]
    out[i] = crop[:, ::-1] if flip[i] else crop
  return out


def bench_host(args):
  from tests import input_ref as R
  rng = np.random.RandomState(0)
  images = rng.randint(0, 256, (N_IMAGES, 32, 32, 3)).astype(np.uint8)
  labels = rng.randint(0, 10, N_IMAGES).astype(np.int32)
  batch = args.batch
  dst = torch.empty(batch, 32, 32, 3, dtype=torch.bfloat16, device=DEV)
  out = {'what': 'host', 'batch': batch, 'host_cpus_used': 1, 'torch_threads': torch.get_num_threads()}
  perm = rng.permutation(N_IMAGES)
  for name, nb, fn in (
      ('numpy_vectorised', args.host_batches, lambda s: torch.from_numpy(_host_batch(images, perm[s * batch:(s + 1) * batch], rng))),
      ('numpy_reference', max(2, args.host_batches // 10),
       lambda s: torch.from_numpy(R.batch(images, labels, batch, s, R.FP32, seed0=1234)[0].view(np.float32)))):
    fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(nb):
      dst.copy_(fn(s))                                 # host fp32 -> device bf16: the copy and the cast
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out[name] = {'batches': nb, 'images_per_s': round(nb * batch / dt, 1), 'ms_per_batch': round(1e3 * dt / nb, 3)}
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--block', type=int, default=100)
  ap.add_argument('--warmup', type=int, default=30)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--chain', type=int, default=100)
  ap.add_argument('--host-batches', type=int, default=50)
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-step', action='store_true')
  ap.add_argument('--skip-launches', action='store_true')
  ap.add_argument('--skip-host', action='store_true')
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('input_bench: no GPU visible; nothing is measured without one')
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
  if not args.skip_host:
    bench_host(args)


if __name__ == '__main__':
  main()
