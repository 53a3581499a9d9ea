"""Per-step training summaries: the scalars every training driver of the reference logs on every step
(rigl/imagenet_resnet/imagenet_train_eval.py:431-473, rigl/imagenet_resnet/utils.py:59-90; the CIFAR and MNIST drivers log
subsets), produced by ONE read-only HIP pass per step (ops.summary_step) into a ring of records in device memory.

  s = TrainingSummaries(graph, optimizer, ring=256, steps_per_epoch=...).attach()
  ... train (eagerly or through train.GraphedStep: a replayed graph leaves a record per replay) ...
  records, dropped = s.read()            # one synchronisation; the records not returned yet, oldest first
  write_jsonl(path, records)

The pass is enqueued inside the inner optimizer's ``apply_gradients`` -- behind the device learning-rate step, in front of the
first update launch -- so a record holds the weights the gradients were taken at, the gradient the update applies
(``mask * (grad_scale * dense) + weight_decay * w``: the arena holds the DENSE gradient of masked kernels) and this step's
rate.  Calls that apply nothing (RigL's mask-update iterations) leave no record; every global step gets exactly one.

The device keeps its own step counter, which equals ``global_step.value`` in front of every call: a step_state.StepCounter,
kept by that module's protocol.  TrainingSummaries is one of its participants; its ``moved`` keeps the ring's ledger in step.

Everything behind the copy of the ring is host arithmetic (``parse_slot`` / ``make_record`` / ``RingLedger``) and runs without
a GPU.
"""
import collections
import json
import math

import numpy as np
import torch

from rigl_amd import _lib
from rigl_amd import ops
from rigl_amd import train
from rigl_amd import variables as V
from rigl_amd.step_state import StepCounter, int32

HEADER_BYTES = _lib.SUMMARY_HEADER_BYTES
GROUP_BYTES = _lib.SUMMARY_GROUP_BYTES
FLOAT_FIELDS = ('sumsq_g', 'sumsq_w', 'l1_w')
COUNT_FIELDS = ('nz_w', 'mask_ones', 'nonfinite_g')
_F32 = np.float32


def slot_bytes(n_entries):
  """rigl_summary_slot_bytes: the header, the totals and one group per entry, rounded up to 64 bytes."""
  return -(-(HEADER_BYTES + GROUP_BYTES * (int(n_entries) + 1)) // 64) * 64


def parse_slot(buf, n_entries):
  """One slot of the ring (a uint8 array of slot_bytes(n_entries) bytes) -> {'step', 'n_entries', 'loss', 'learning_rate',
  'totals': {field: value}, 'entries': {field: array [n_entries]}}."""
  buf = np.ascontiguousarray(np.asarray(buf, dtype=np.uint8)[:slot_bytes(n_entries)])
  head_i = buf[:8].view(np.int32)
  head_f = buf[8:16].view(np.float32)
  groups = buf[HEADER_BYTES:HEADER_BYTES + GROUP_BYTES * (n_entries + 1)].reshape(n_entries + 1, GROUP_BYTES)
  f = np.ascontiguousarray(groups[:, :24]).view(np.float64).reshape(n_entries + 1, 3)
  c = np.ascontiguousarray(groups[:, 24:]).view(np.int64).reshape(n_entries + 1, 3)
  out = {'step': int(head_i[0]), 'n_entries': int(head_i[1]), 'loss': float(head_f[0]), 'learning_rate': float(head_f[1]),
         'totals': {}, 'entries': {}}
  for k, name in enumerate(FLOAT_FIELDS):
    out['totals'][name] = float(f[0, k])
    out['entries'][name] = f[1:, k].copy()
  for k, name in enumerate(COUNT_FIELDS):
    out['totals'][name] = int(c[0, k])
    out['entries'][name] = c[1:, k].copy()
  return out


def _mask_key(mask_name):
  name = mask_name[:-2] if mask_name.endswith(':0') else mask_name         # the op name, as evaluation.sparsity_metrics
  return 'pruning/%s/sparsity' % name


def make_record(rec, layout, steps_per_epoch=None, drop_fraction=None, per_variable=False):
  """The reference's scalars from one parsed slot.  ``layout``: one dict per entry, in table order, with 'name', 'n',
  'weight_decay' (the VARIABLE's own, whatever the update applied) and 'mask' (the mask variable's name, or None).
  ``drop_fraction``: callable step -> float, or None."""
  if rec['n_entries'] != len(layout):
    raise ValueError('the record has %d entries, the layout %d' % (rec['n_entries'], len(layout)))
  ent, tot = rec['entries'], rec['totals']
  step = rec['step']
  reg = 0.0                                           # evaluation.reg_loss: sum of decay * sum(w^2) / 2, in fp64
  for i, l in enumerate(layout):
    if l['weight_decay'] > 0.0:
      reg += l['weight_decay'] * float(ent['sumsq_w'][i]) / 2.0
  cross = rec['loss']
  out = {'global_step': step, 'loss': cross + reg, 'cross_loss': cross, 'reg_loss': reg, 'learning_rate': rec['learning_rate']}
  if steps_per_epoch is not None:
    out['current_epoch'] = step / float(steps_per_epoch)
  if drop_fraction is not None:
    out['drop_fraction'] = float(drop_fraction(step))
  out['grad_norm'] = math.sqrt(tot['sumsq_g']) if tot['sumsq_g'] == tot['sumsq_g'] else float('nan')
  out['var_norm'] = math.sqrt(tot['sumsq_w']) if tot['sumsq_w'] == tot['sumsq_w'] else float('nan')
  out['grad_nonfinite'] = tot['nonfinite_g']
  masked = [i for i, l in enumerate(layout) if l['mask'] is not None]
  if masked:
    i0 = masked[0]                                    # pruning.get_weights()[0] / get_masks()[0]
    out['fw_nz_weight'] = int(ent['nz_w'][i0])
    out['fw_nz_mask'] = int(ent['mask_ones'][i0])
    out['fw_l1_weight'] = float(ent['l1_w'][i0])
    dense = ones = 0.                                 # sparse_utils.calculate_sparsity, on the counts
    for i in masked:
      dense += float(layout[i]['n'])
      ones += float(int(ent['mask_ones'][i]))
    out['global_sparsity'] = 1. - ones / dense
    for i in masked:                                  # pruning.get_weight_sparsity: fp32
      sp = _F32(1) - _F32(_F32(int(ent['mask_ones'][i])) / _F32(layout[i]['n']))
      out[_mask_key(layout[i]['mask'])] = float(sp)
  if per_variable:
    out['per_variable'] = {
        l['name']: dict([(k, float(ent[k][i])) for k in FLOAT_FIELDS] + [(k, int(ent[k][i])) for k in COUNT_FIELDS])
        for i, l in enumerate(layout)}
  return out


def mask_summaries(masks, with_img=False):
  """rigl/imagenet_resnet/utils.py:83-90 on mask variables, read from the device now (one popcount per mask):
  {'pruning/<mask op name>/sparsity': tf.nn.zero_fraction(mask)} in fp32 arithmetic.  Mask images are not produced."""
  if with_img:
    raise NotImplementedError('mask_summaries(with_img=True): image summaries have no counterpart here')
  return {_mask_key(m.name): float(_F32(1) - _F32(_F32(m.sum()) / _F32(m.numel))) for m in masks}


class RingLedger:
  """What the ring holds, kept on the host: the device writes step s into slot s mod ``slots`` -- a write to a slot whose
  record was not read yet drops that record.  ``take()`` returns the steps whose records are alive, in the order they were
  written, and how many were dropped since the last take."""

  def __init__(self, slots):
    if slots < 1:
      raise ValueError('a ring needs at least 1 slot, got %d' % slots)
    self.slots = int(slots)
    self._live = collections.OrderedDict()            # slot -> step, oldest write first
    self._dropped = 0
    self._last = None                                 # (slot, the step it replaced or None): undo of the newest write

  def slot_of(self, step):
    return int32(step) % self.slots                  # python's % is non-negative: what the kernel computes

  def wrote(self, step):
    slot = self.slot_of(step)
    before = self._live.pop(slot, None)
    if before is not None:
      self._dropped += 1
    self._live[slot] = int32(step)
    self._last = (slot, before)

  def undo(self):
    """The newest ``wrote`` did not happen (a stream capture enqueues nothing).  Only the newest can be undone; a record it
    displaced comes back at the end of the order."""
    if self._last is None:
      raise RuntimeError('RingLedger.undo: nothing to undo')
    slot, before = self._last
    del self._live[slot]
    if before is not None:
      self._live[slot] = before
      self._dropped -= 1
    self._last = None

  def take(self):
    live, dropped = list(self._live.items()), self._dropped
    self._live.clear()
    self._dropped = 0
    self._last = None
    return live, dropped


def write_jsonl(path, records, append=True):
  """One JSON object per record and line.  Non-finite numbers are written as JSON strings ('nan', 'inf', '-inf')."""
  def clean(v):
    if isinstance(v, dict):
      return {k: clean(x) for k, x in v.items()}
    if isinstance(v, float) and not math.isfinite(v):
      return repr(v)
    if isinstance(v, (np.floating, np.integer)):
      return clean(v.item())
    return v
  with open(path, 'a' if append else 'w') as f:
    for r in records:
      f.write(json.dumps(clean(r), sort_keys=True) + '\n')


class TrainingSummaries:
  """See the module docstring.  ``optimizer``: the optimizer the training loop calls -- an inner GradientDescentOptimizer /
  MomentumOptimizer / AdamOptimizer or a sparse wrapper around one (its ``_optimizer``); ``ring``: slots of the device ring."""

  def __init__(self, graph, optimizer, ring=256, steps_per_epoch=None):
    self._graph = graph
    self._outer = optimizer
    self._inner = train.inner_optimizer(optimizer)
    if not hasattr(self._inner, 'summary_hook'):
      raise TypeError('%s has no summary hook (expected a rigl_amd.train optimizer)' % type(self._inner).__name__)
    self._steps_per_epoch = steps_per_epoch
    self._ledger = RingLedger(ring)
    graph.finalize()
    if graph.W is None or not graph.W.is_cuda:
      raise _lib.RiglError(_lib.RIGL_EINVAL, 'training summaries need a graph on the GPU (no CPU path exists)')
    self.counter = StepCounter(graph.W.device, "summaries'")
    self._build()
    graph.add_relayout_callback(self._build)

  # ---- the entry table ---------------------------------------------------------------------------------------------------
  def _build(self):
    """(Re)builds the layout and both tables from the graph's arenas; a relayout starts an empty ring."""
    g = self._graph
    masks = {l.weights.name: l.mask for l in g.layers if l.mask is not None}
    order = sorted(g.trainable_variables(), key=lambda v: v.offset)
    self.layout, self._tables, self._keep = [], {}, []
    rows = {False: [], True: []}                      # keyed by the optimizer's dense_masked_update
    for v in order:
      m = masks.get(v.name)
      w = g.W[v.offset:v.offset + v.numel]
      gr = g.G[v.offset:v.offset + v.numel]
      bits = m.bits if m is not None else None
      wd = v.weight_decay if v.kind in (V.KIND_MASKED, V.KIND_DENSE) else 0.0   # what apply_gradients hands the update
      self.layout.append({'name': v.name, 'n': v.numel, 'weight_decay': v.weight_decay,
                          'mask': m.name if m is not None else None})
      rows[False].append((w, gr, bits, wd, 1))
      rows[True].append((w, gr, bits, 0.0 if m is not None else wd, 0 if m is not None else 1))   # DNW: dense, undecayed
      self._keep.append((w, gr, bits))
    for dense, r in rows.items():
      self._tables[dense] = ops.summary_table(r)
    self._slot_bytes = ops.summary_slot_bytes(len(order))
    assert self._slot_bytes == slot_bytes(len(order))
    self._ring = torch.zeros(self._ledger.slots * self._slot_bytes, dtype=torch.uint8, device=g.W.device)
    self._ledger = RingLedger(self._ledger.slots)

  # ---- the hook ----------------------------------------------------------------------------------------------------------
  def attach(self):
    self._inner.summary_hook = self
    return self

  def detach(self):
    if self._inner.summary_hook is self:
      self._inner.summary_hook = None

  def fresh(self, global_step):
    return self.counter.fresh(global_step)

  def moved(self, k):
    """The device counter moved by ``k``: +1 a launch of the hook or a graph replay (either wrote a record), -1 undoing the
    host side of a capture (which wrote none)."""
    if k == 1:
      self._ledger.wrote(self.counter.mirror)
    elif k == -1:
      self._ledger.undo()
    else:
      raise ValueError('moved: k must be +1 or -1')
    self.counter.moved(k)

  def on_apply(self, global_step, loss, lr, grad_scale):
    """Called by the inner optimizer's apply_gradients: behind the device learning-rate step, in front of the first update
    launch.  ``loss``: the step's (GradientDescentOptimizer.step_loss); ``lr``: a float, or the device rate's tensor."""
    self.counter.sync(global_step)
    ops.summary_step(self._tables[bool(self._inner.dense_masked_update)], self.counter.tensor, self._ring, self._ledger.slots,
                     grad_scale=grad_scale, loss=loss, **ops.lr_kwargs(lr))
    self.moved(1)

  # ---- reading -----------------------------------------------------------------------------------------------------------
  def _drop_fraction(self):
    o = self._outer
    if hasattr(o, 'get_drop_fraction'):
      return lambda step: o.get_drop_fraction(step, True)   # the annealed fraction a mask update at that step uses
    return None

  def read(self, per_variable=False):
    """Synchronises once, copies the ring and returns (records, dropped): the records not returned yet, oldest first, as
    dicts keyed by the reference's names, and the number of steps overwritten before they were read."""
    live, dropped = self._ledger.take()
    if not live:
      return [], dropped
    host = self._ring.cpu().numpy()                   # (the copy synchronises with the stream)
    out = []
    for slot, step in live:
      rec = parse_slot(host[slot * self._slot_bytes:(slot + 1) * self._slot_bytes], len(self.layout))
      if rec['step'] != step:
        raise RuntimeError('ring slot %d holds step %d, the host expected %d' % (slot, rec['step'], step))
      out.append(make_record(rec, self.layout, self._steps_per_epoch, self._drop_fraction(), per_variable))
    return out, dropped
