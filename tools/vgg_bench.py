"""VGG RigL training step on one GPU: images/s and ms/step, K1 (the masked conv kernels) achieved FLOP/s and its share of
the 2.5 PFLOP/s dense bf16 peak, and the A/B of the fused ReLU epilogues against the stand-alone ReLU passes.

One step = SparseRigLOptimizer(MomentumOptimizer, Nesterov 0.9).minimize on a batch of synthetic 224 x 224 images, ERK 0.8,
drop fraction 0.3; the schedule is positioned so that exactly one mask update falls inside every timed window.  Times come
from device events around the window (a synchronise at its end).  K1 time is the per-launch time the library records for its
conv kernels (rigl_prof_*, in a separate window: the stamped launches cost a little), FLOPs are computed from the layer
shapes: 2 x MACs for forward, dgrad (not conv1_1) and wgrad of every conv and of fc8.

  python tools/vgg_bench.py                          # vgg_16 and vgg_a, fused (the default) -- one JSON line per model
  python tools/vgg_bench.py --ab 4 --models vgg_16   # + fused / stand-alone (knob relu_fuse) alternating, 4 windows each
Run rocprofv3 --kernel-trace --stats on it in a run of its own (--steps small).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BF16 = 2.5e15
PERIOD = 100


def build(vgg_type, batch, image_size, dev):
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import vgg
  g = V.reset_default_graph(dev)
  model = vgg.VGG(vgg_type, num_classes=1000, weight_decay=5e-4, seed=0, graph=g)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  inner = train.MomentumOptimizer(0.1 * batch / 256.0, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 100000, PERIOD, drop_fraction=0.3, drop_fraction_anneal='constant')
  gs = g.get_or_create_global_step()
  images, labels = vgg.synthetic_batch(batch, dev, seed=1234, image_size=image_size)

  def step():
    loss = model.loss(images, labels, label_smoothing=0.1)
    opt.minimize(loss, gs)
    return loss
  return step, gs


def flops_per_step(vgg_type, batch, image_size):
  from rigl_amd.workloads import shapes as WS
  fwd, dgrad, fc8 = WS.vgg_macs_per_image(vgg_type, image_size)
  return 2.0 * batch * (2 * fwd + dgrad + 3 * fc8)     # fwd + wgrad of every conv, dgrad of all but conv1_1, fc8 fwd/dgrad/wgrad


def timed_window(step, gs, steps):
  """`steps` steps with one mask update among them (the update is call 1 of the window)."""
  gs.value = (int(gs.value) // PERIOD + 1) * PERIOD - 1   # call 0: an ordinary step; call 1: the mask update
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(steps):
    loss = step()
  b.record()
  torch.cuda.synchronize()
  assert np.isfinite(float(loss.detach().float()))
  return a.elapsed_time(b) / steps


def measure(vgg_type, args, dev):
  from rigl_amd import ops
  step, gs = build(vgg_type, args.batch, args.image_size, dev)
  for _ in range(args.warmup):
    step()
  torch.cuda.synchronize()
  ms = timed_window(step, gs, args.steps)
  ops.prof_enable(True)
  ops.prof_collect()
  timed_window(step, gs, args.steps)
  prof = ops.prof_collect()
  ops.prof_enable(False)
  k1_ms = sum(prof[k][0] for k in ('conv_fwd', 'conv_dgrad', 'conv_wgrad', 'conv_bwd')) / args.steps
  fl = flops_per_step(vgg_type, args.batch, args.image_size)
  out = dict(model=vgg_type, batch=args.batch, image_size=args.image_size, steps=args.steps, ms_per_step=round(ms, 3),
             images_per_s=round(args.batch * 1000.0 / ms, 1), step_tflop=round(fl / 1e12, 3),
             k1_ms_per_step=round(k1_ms, 3), k1_tflops=round(fl / (k1_ms * 1e-3) / 1e12, 1),
             k1_peak_share=round(fl / (k1_ms * 1e-3) / PEAK_BF16, 3),
             step_peak_share=round(fl / (ms * 1e-3) / PEAK_BF16, 3))
  if args.ab:
    rows = {'fused': [], 'standalone': []}
    for _ in range(args.ab):
      for name, knob in (('fused', 1), ('standalone', 0)):
        ops.tune_set('relu_fuse', knob)
        step()                                     # (re-plans after the knob change; not timed)
        rows[name].append(round(timed_window(step, gs, args.steps), 3))
    ops.tune_unset('relu_fuse')
    out['ab_ms_per_step'] = rows
    out['ab_median'] = {k: float(np.median(v)) for k, v in rows.items()}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--models', default='vgg_16,vgg_a')
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--image-size', type=int, default=224)
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--ab', type=int, default=0, help='fused / stand-alone windows, alternating')
  ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('vgg_bench: needs a GPU (no CPU measurement path)')
  dev = 'cuda:0'
  for m in args.models.split(','):
    t0 = time.time()
    r = measure(m, args, dev)
    r['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(r)
    print(line, flush=True)
    if args.out:
      with open(args.out, 'a') as f:
        f.write(line + '\n')


if __name__ == '__main__':
  main()
