#!/usr/bin/env python3
"""Worker of tests/test_accum_dp_gpu.py: train.MicroBatches together with the data-parallel exchange (dist.GradSync).

  python tests/accum_dp_worker.py --case forced --model mlp --port 29601 --out f.json
      ONE rank, a gloo group of one, the exchange forced on (GradSync(enabled=True)), k = 3: five calls (global steps 0 and 2
      are mask updates), then the same run with grad_sync=None, a plain data-parallel run (no MicroBatches) and one through
      MicroBatches(..., 1).  Writes a digest of W, the mask bitmap, the momentum slots and G after every call of the first two
      runs, the collectives and accumulate launches counted in every run, and the kernel launch counts of the last two.
  python -m torch.distributed.run --nproc-per-node 2 ... tests/accum_dp_worker.py --case two --model mlp --out f.json
      TWO ranks, k = 2 (``--backend gloo``: both on cuda:0; ``nccl``: one device each).  Every rank first computes S_0 and S_1,
      the arena of a MicroBatches(k = 2) run WITHOUT an exchange on rank 0's and on rank 1's micro-batches, then runs five
      calls with the exchange: after call 0's compute_gradients the arena must be fl(S_0 + S_1); the masks are compared across
      ranks after every call.  Then every rank runs ONE rank x k = 4 on the same four micro-batches per call.  Rank 0 writes.

Collectives are counted by wrapping torch.distributed.all_reduce; accumulate launches by wrapping ops.grad_accumulate and
ops.grad_accumulate_ranges.  Micro-batch j of call s is seeded by (s, j) alone: rank r of a k-per-rank run takes j = r * k + i.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

CALLS = 5
COUNT = {'all_reduce': 0, 'accumulate': 0, 'accumulate_ranges': 0}
MODELS = {'mlp': dict(batch=32, bucket_bytes=4096, lr=0.2), 'wrn': dict(batch=16, bucket_bytes=65536, lr=0.05)}


def _wrap_counters():
  from rigl_amd import ops
  real_ar, real_acc, real_rng = dist.all_reduce, ops.grad_accumulate, ops.grad_accumulate_ranges

  def all_reduce(*a, **kw):
    COUNT['all_reduce'] += 1
    return real_ar(*a, **kw)

  def grad_accumulate(*a, **kw):
    COUNT['accumulate'] += 1
    return real_acc(*a, **kw)

  def grad_accumulate_ranges(*a, **kw):
    COUNT['accumulate_ranges'] += 1
    return real_rng(*a, **kw)
  dist.all_reduce, ops.grad_accumulate, ops.grad_accumulate_ranges = all_reduce, grad_accumulate, grad_accumulate_ranges


def micro_batch(model, dev, call, j):
  gen = torch.Generator(device='cpu').manual_seed(100000 + 64 * call + j)
  b = MODELS[model]['batch']
  if model == 'mlp':
    x = torch.rand(b, 784, generator=gen).to(torch.bfloat16)
  else:
    x = torch.randn(b, 8, 8, 3, generator=gen).to(torch.bfloat16)
  y = torch.randint(0, 10, (b,), generator=gen)
  return x.to(dev), y.to(dev)


class Run:
  """One freshly built model, optimizer and (optionally) exchange; ``call(s)`` is one optimizer call on call s's micro-batches
  first .. first + k - 1."""

  def __init__(self, model, dev, k, first=0, sync='none', micro_batches=True):
    from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
    from rigl_amd.dist import GradSync
    from rigl_amd.workloads import mnist_mlp, wide_resnet
    self.name, self.dev, self.k, self.first = model, dev, k, first
    self.g = g = V.reset_default_graph(dev)
    if model == 'mlp':
      self.model = mnist_mlp.MnistMLP(g, seed=0)
      np.random.seed(0)
      sparse_utils.get_mask_init_fn(g.get_masks(), 'random', 0.9, {'layer3': 0.0})()
    else:
      # two blocks per group, 8 x 8 images; the stem masked too: a dense kernel lies BEHIND the masked ones in the arena while
      # its gradient comes last, and no bucket could leave before the flush
      self.model = wide_resnet.WideResNet(g, depth=16, width=1, seed=0, prune_first_layer=True)
      np.random.seed(0)
      sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
    cfg = MODELS[model]
    self.sync = None
    if sync != 'none':
      self.sync = GradSync(g, bucket_bytes=cfg['bucket_bytes'], enabled=True if sync == 'forced' else None)
    self.inner = train.MomentumOptimizer(cfg['lr'], 0.9, use_nesterov=True, graph=g, grad_sync=self.sync)
    self.opt = SO.SparseRigLOptimizer(self.inner, 0, 50000, 2, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.,
                                      use_tpu=self.sync is not None)
    self.gs = g.get_or_create_global_step()
    self._call = 0
    self._i = 0
    self.at_pass = []              # the collectives counted so far, at every loss_fn call of the current optimizer call
    self.fn = train.MicroBatches(self._loss_fn, self.opt, micro_batches=k) if micro_batches else self._loss_fn

  def _loss_fn(self):
    self.at_pass.append(COUNT['all_reduce'])
    x, y = micro_batch(self.name, self.dev, self._call, self.first + self._i)
    self._i += 1
    return self.model.loss(x, y)

  def begin(self, s):
    self._call, self._i, self.at_pass = s, 0, []
    return self.fn()

  def call(self, s):
    """One optimizer call; returns what it enqueued: collectives in all, collectives before the k-th pass began, accumulate
    launches, the bytes of the step's exchange timeline and its number of collective launches."""
    c0 = dict(COUNT)
    loss = self.begin(s)
    self.opt.minimize(loss, self.gs)
    return self.counted(c0)

  def counted(self, c0):
    out = {k: COUNT[k] - c0[k] for k in COUNT}
    out['held'] = self.at_pass[-1] - self.at_pass[0]
    out['passes'] = len(self.at_pass)
    if self.sync is not None:
      tl = self.sync.timeline_summary()
      out['timeline_bytes'] = sum(r['bytes'] for r in tl['buckets']) if tl else 0
      out['arena_bytes'] = 4 * self.g.G.numel()
      out['launches'] = self.sync.n_buckets_last
    return out

  def digests(self):
    torch.cuda.synchronize()
    h = lambda t: 'none' if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    return dict(W=h(self.g.W), BITS=h(self.g.BITS), slot=h(self.inner._slot), G=h(self.g.G), gs=int(self.gs.value))   # pylint: disable=protected-access

  def mean_loss(self):
    l = self.fn.loss.detach().float().reshape(1).clone()
    if self.sync is not None and self.sync.world > 1:
      if dist.get_backend() == 'gloo':
        l = l.cpu()
      dist.all_reduce(l)
      l /= self.sync.world
    return float(l.item())

  def summary(self):
    return dict(w_norm=float(self.g.W.double().norm().item()), mask_ones=[int(m.sum()) for m in self.g.get_masks()],
                global_step=int(self.gs.value))


def _launch_counts(run, s):
  """The kernel launches per kind of one call (the library's profiler), after one call that lets buffers settle."""
  from rigl_amd import ops
  torch.cuda.synchronize()
  ops.prof_enable(True)
  try:
    ops.prof_collect()
    counted = run.call(s)
    return {k: v[1] for k, v in ops.prof_collect().items()}, counted
  finally:
    ops.prof_enable(False)


def case_forced(a, dev):
  os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
  os.environ['MASTER_PORT'] = str(a.port)
  dist.init_process_group('gloo', rank=0, world_size=1)
  out = {'world': 1, 'backend': dist.get_backend(), 'k': 3}
  for name, sync in (('exchange', 'forced'), ('alone', 'none')):
    run = Run(a.model, dev, 3, sync=sync)
    rows = []
    for s in range(CALLS):
      counted = run.call(s)
      rows.append(dict(run.digests(), loss=run.mean_loss(), **counted))
    out[name] = rows
    if run.sync is not None:
      out['enabled'], out['grad_scale'] = bool(run.sync.enabled), run.sync.grad_scale
  # a plain data-parallel run and one through MicroBatches(..., 1): calls 0 (a mask update) and 1 settle, call 2 is counted
  for name, mb in (('plain', False), ('k1', True)):
    run = Run(a.model, dev, 1, sync='forced', micro_batches=mb)
    rows = [run.call(s) for s in range(2)]
    launches, counted = _launch_counts(run, 2)
    rows.append(counted)
    out[name] = dict(calls=rows, launches=launches, digests=run.digests(),
                     arena=None if not mb else (run.fn._arena is None))   # pylint: disable=protected-access
  dist.destroy_process_group()
  return out


def case_two(a, dev):
  world, rank = int(os.environ['WORLD_SIZE']), int(os.environ['RANK'])
  os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
  if a.backend == 'gloo':
    dist.init_process_group('gloo', rank=rank, world_size=world)
  else:
    dist.init_process_group('nccl', device_id=dev, rank=rank, world_size=world)
  k = 2
  out = {'world': world, 'backend': dist.get_backend(), 'k': k}
  # S_r: the arena of an accumulated call WITHOUT an exchange on rank r's micro-batches, from the common initial state
  S = []
  for r in range(world):
    run = Run(a.model, dev, k, first=r * k)
    run.inner.compute_gradients(run.begin(0))
    S.append(run.g.G.detach().clone())
  want = S[0] + S[1]                                  # one fp32 addition per element
  run = Run(a.model, dev, k, first=rank * k, sync='auto')
  rows, same = [], []
  for s in range(CALLS):
    c0 = dict(COUNT)
    loss = run.begin(s)
    if s == 0:
      run.inner.compute_gradients(loss)
      got = run.g.G.detach()
      diff = (got.view(torch.int32) != want.view(torch.int32))
      t = torch.tensor([int(diff.sum().item())], dtype=torch.int64, device=dev if a.backend == 'nccl' else 'cpu')
      real = dist.all_reduce
      real(t, op=dist.ReduceOp.MAX)
      COUNT['all_reduce'] -= 1                        # (the check's own collective)
      out['g_words_differing_from_fl_S0_plus_S1'] = int(t.item())
      out['g_words'] = int(got.numel())
      out['S_differ'] = int((S[0].view(torch.int32) != S[1].view(torch.int32)).sum().item())
      out['update_scale'] = run.inner.update_scale()
    run.opt.minimize(loss, run.gs)
    counted = run.counted(c0)
    rows.append(dict(loss=run.mean_loss(), gs=int(run.gs.value), **counted))
    same.append(bool(run.sync.check_masks_identical()))
  out['calls'], out['masks_identical'] = rows, same
  out['two'] = run.summary()
  plain = Run(a.model, dev, 1, first=rank, sync='auto', micro_batches=False)
  out['plain_calls'] = [plain.call(s) for s in range(3)]
  # one rank x k = 4 on the same four micro-batches of every call
  one = Run(a.model, dev, 2 * k)
  losses = []
  for s in range(CALLS):
    one.call(s)
    losses.append(one.mean_loss())
  out['one'] = dict(one.summary(), losses=losses)
  dist.barrier()
  dist.destroy_process_group()
  return out if rank == 0 else None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--case', choices=['forced', 'two'], required=True)
  ap.add_argument('--model', choices=sorted(MODELS), required=True)
  ap.add_argument('--backend', choices=['gloo', 'nccl'], default='gloo')
  ap.add_argument('--port', type=int, default=29601)
  ap.add_argument('--out', required=True)
  a = ap.parse_args()
  local = int(os.environ.get('LOCAL_RANK', '0')) if (a.case == 'two' and a.backend == 'nccl') else 0
  torch.cuda.set_device(local)
  dev = torch.device('cuda', local)
  _wrap_counters()
  out = case_forced(a, dev) if a.case == 'forced' else case_two(a, dev)
  if out is not None:
    with open(a.out, 'w') as fh:
      json.dump(out, fh)


if __name__ == '__main__':
  main()
